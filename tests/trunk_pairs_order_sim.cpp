// Host-only simulation of the trunk kernel's workgroup streams with blocking neighbourhood waits
// (tests/test_trunk_pairs_order_cpu.py compiles and runs it): does a launch of G workgroups over
// n x nby x nbx tiles run to completion when growth pairs are run pair-major?
//
// The model follows trunk.hip: workgroup b owns tiles b, b + G, ...; progress[t] = layers done on
// tile t; the layers are two RDBs (conv0..conv3 growth, conv4 final).  An unpaired item (l, t) waits
// until every tile of t's 3x3 neighbourhood (same image) has progress >= l, then publishes l + 1.
// A pair (l, l + 1) is, per tile, phase 1 (waits for l, publishes l + 1) followed at once by phase 2
// (waits for l + 1, publishes l + 2).  The last chunk of an item also stages the next item's chunk 0:
// when the next layer's first chunk is one its previous layer wrote (conv0 of an RDB after the first)
// and the next tile is not adjacent, the item waits for the NEXT item's neighbourhood before it
// publishes itself.  Waits are monotone, so the order in which workgroups are stepped is irrelevant:
// a sweep that advances nobody is a deadlock.
//
// Output: one line per geometry: n nbx nby G allowed unpaired_done paired_done
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "trunk_pairs.h"

namespace {

constexpr int kLayers = 10;  // two RDBs

struct Geo {
    int n, nbx, nby, G;
    int ntiles() const { return n * nbx * nby; }
};

bool adjacent(const Geo& g, int t, int t2) {
    const int bx = t % g.nbx, tq = t / g.nbx, by = tq % g.nby, im = tq / g.nby;
    const int bx2 = t2 % g.nbx, nq = t2 / g.nbx, by2 = nq % g.nby, im2 = nq / g.nby;
    return im == im2 && abs(bx - bx2) <= 1 && abs(by - by2) <= 1;
}

bool neighbourhood_at(const Geo& g, const std::vector<int>& progress, int t, int need) {
    const int bx = t % g.nbx, tq = t / g.nbx, by = tq % g.nby, im = tq / g.nby;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int yy = by + dy, xx = bx + dx;
            if (yy < 0 || yy >= g.nby || xx < 0 || xx >= g.nbx) continue;
            if (progress[(size_t)(im * g.nby + yy) * g.nbx + xx] < need) return false;
        }
    return true;
}

struct Item {
    int layer, tile;
    bool prefetch_next;  // its last chunk may block on the next item's neighbourhood
};

// the stream of workgroup b (trunk_kernel's item loop and next_item)
std::vector<Item> stream_of(const Geo& g, int b, bool paired) {
    std::vector<Item> s;
    for (int l = 0; l < kLayers;) {
        const int k = l % 5;
        const bool pair = paired && (k == 0 || k == 2);
        for (int t = b; t < g.ntiles(); t += g.G) {
            s.push_back({l, t, !pair});
            if (pair) s.push_back({l + 1, t, true});  // phase 2 directly behind phase 1 of the tile
        }
        l += pair ? 2 : 1;
    }
    return s;
}

bool run(const Geo& g, bool paired) {
    const int nt = g.ntiles();
    std::vector<int> progress((size_t)nt, 0);
    const int nwg = g.G < nt ? g.G : nt;
    std::vector<std::vector<Item>> streams;
    for (int b = 0; b < nwg; ++b) streams.push_back(stream_of(g, b, paired));
    std::vector<size_t> pc((size_t)nwg, 0);
    std::vector<char> deps_met((size_t)nwg, 0);
    for (;;) {
        bool moved = false, all_done = true;
        for (int b = 0; b < nwg; ++b) {
            const std::vector<Item>& s = streams[(size_t)b];
            while (pc[(size_t)b] < s.size()) {
                const Item& it = s[pc[(size_t)b]];
                if (!deps_met[(size_t)b]) {
                    if (it.layer > 0 && !neighbourhood_at(g, progress, it.tile, it.layer)) break;
                    deps_met[(size_t)b] = 1;
                    moved = true;
                }
                if (it.prefetch_next && pc[(size_t)b] + 1 < s.size()) {
                    const Item& nx = s[pc[(size_t)b] + 1];
                    const bool first_chunk_is_new = nx.layer > 0 && nx.layer % 5 == 0;
                    if (first_chunk_is_new && !adjacent(g, it.tile, nx.tile) &&
                        !neighbourhood_at(g, progress, nx.tile, nx.layer))
                        break;
                }
                progress[(size_t)it.tile] = it.layer + 1;
                ++pc[(size_t)b];
                deps_met[(size_t)b] = 0;
                moved = true;
            }
            if (pc[(size_t)b] < s.size()) all_done = false;
        }
        if (all_done) return true;
        if (!moved) return false;
    }
}

void report(const Geo& g) {
    const bool allowed = isr::pairs_allowed(g.ntiles(), g.nbx, g.nby, g.n, g.G);
    std::printf("%d %d %d %d %d %d %d\n", g.n, g.nbx, g.nby, g.G, (int)allowed, (int)run(g, false), (int)run(g, true));
}

}  // namespace

int main() {
    for (int n = 1; n <= 2; ++n)
        for (int nbx = 1; nbx <= 10; ++nbx)
            for (int nby = 1; nby <= 4; ++nby)
                for (int G = 1; G <= 2 * (nbx + 2) + 3; ++G) report({n, nbx, nby, G});
    // launches of the size the kernel runs at (512 workgroups): 546 tiles, the 768-tile row of 256,
    // a 1080p frame (4,080 tiles), and the same frame on a grid just below and at the rule's edge
    const Geo big[] = {{3, 13, 14, 512}, {1, 256, 3, 512}, {1, 60, 68, 512}, {1, 60, 68, 123}, {1, 60, 68, 124},
                       {1, 60, 68, 61},  {1, 60, 68, 60}};
    for (const Geo& g : big) report(g);
    return 0;
}
