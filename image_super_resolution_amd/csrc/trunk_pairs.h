// When the persistent trunk kernel (trunk.hip) may run two growth convs of an RDB as one pair item
// per tile.  No HIP dependency: the prep kernel and a host-only simulation (tests/
// test_trunk_pairs_order_cpu.py) include the same rule.
//
// A pair (A = layer L, B = layer L + 1) turns a workgroup's stream for those two layers from
// layer-major (A on every tile of the workgroup, then B on every tile) into pair-major: for each
// tile t = b, b + G, ...: phase 1 (A and B on the chunks they share), then phase 2 (B on the two
// chunks A just wrote).  Phase 2 always follows phase 1 of the same tile, so the tile's own pixels
// of those two chunks can stay in LDS (trunk_keep.h) and phase 2 reads only the ring of halo
// pixels its neighbours wrote: that changes what phase 2 fetches after its wait, not what it waits
// for.  The blocking waits inside one pair are
//   P2(a)  -> P1(a')      a' in the 3x3 neighbourhood of a (a itself included): a' <= a + nbx + 1
//   P1(a') -> P2(a' - G)  the item before it in its workgroup's stream (when a' >= G)
//   P2(a)  -> P2(n)       a the last tile of workgroup b with a >= b + G, n in the neighbourhood of
//                         b: the last chunk of a stream's last tile waits for the first tile of
//                         the next layer before it stages that tile's chunk 0; n <= b + nbx + 1
// and every other wait is for a layer before the pair, which never waits for the pair.  With
// ntiles <= G a workgroup owns one tile and only the first kind exists: P1 waits for nothing in
// the pair.  With ntiles > G and nbx + 2 <= G every path P2 -> ... -> P2 and P1 -> ... -> P1 ends
// on a strictly smaller tile index (a' - G <= a + nbx + 1 - G < a; n <= a - G + nbx + 1 < a), so
// the wait graph has no cycle; at G == nbx + 1, nbx or nbx - 1 tile a waits for P1(a + G), which
// its own workgroup runs after P2(a): a deadlock.  The rule asks for twice that margin,
// 2 (nbx + 2) <= G: every hop of a wait chain inside a pair then moves down by more than G / 2
// tiles, so a chain is at most 2 ntiles / G hops long and pairing cannot serialise the grid or
// come near the bounded spin.  Where the rule says no, the stream is the unpaired one.
#pragma once

namespace isr {

#if defined(__HIP__) || defined(__CUDACC__)
#define ISR_PAIRS_HD __host__ __device__
#else
#define ISR_PAIRS_HD
#endif

// ntiles = n * nby * nbx tiles (nbx per tile row), G = workgroups of the launch.
static inline ISR_PAIRS_HD bool pairs_allowed(long long ntiles, int nbx, int nby, int n, int G) {
    if (ntiles <= 0 || nbx <= 0 || nby <= 0 || n <= 0 || G <= 0) return false;
    if (ntiles <= G) return true;
    return 2ll * (nbx + 2) <= G;
}

// Values of the host switch ISR_TRUNK_PAIRS (read once by the launch, passed to the prep kernel).
enum : int {
    TRUNK_PAIRS_OFF = 0,   // no pairs: the per-layer stream
    TRUNK_PAIRS_LONG = 1,  // only pairs that share 8 chunks or more: (conv2, conv3) of an RDB
    TRUNK_PAIRS_ALL = 2    // every pair
};

}  // namespace isr
