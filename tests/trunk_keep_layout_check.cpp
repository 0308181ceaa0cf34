// Host-only check of the kept-tile layout of the trunk kernel (csrc/trunk_keep.h;
// tests/test_trunk_keep_layout_cpu.py compiles and runs it, plain and under ASan + UBSan).
//
// For wp in {36, 54, 130, 8194} (pixels per buffer row), exhaustively:
//  * every epilogue register (4 waves x 4 rows x 32 lanes x 2 channel halves) lands on the LDS unit
//    whose LDS-DMA source (halo_unit_src, what trunk_common.h halo_piece_off returns) is that pixel
//    and channel half of the plane;
//  * the 1,024 interior units and the 200 ring units are disjoint and together exactly the units of
//    the pixels q < 612;
//  * each ring unit's source offset is halo_unit_src of that unit.
// Output: one line per wp: wp interior ring covered; exit status 1 and a message on a violation.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "trunk_keep.h"

namespace {

int fail(const char* what, int wp, int a, int b) {
    std::fprintf(stderr, "wp %d: %s (%d, %d)\n", wp, what, a, b);
    return 1;
}

int check(int wp) {
    using namespace isr;
    const int units = 2 * keep::HQ;
    std::vector<int> owner(units, 0);  // 0 nobody, 1 interior, 2 ring
    int interior = 0, ring = 0;
    for (int wave = 0; wave < 4; ++wave)
        for (int r = 0; r < keep::ROWS_PER_WAVE; ++r)
            for (int l31 = 0; l31 < 32; ++l31)
                for (int hh = 0; hh < 2; ++hh) {
                    const uint32_t off = keep_epi_lds_off(wave, r, l31, hh);
                    if (off % 16 || off / 16 >= (uint32_t)units) return fail("epilogue offset outside the image", wp, wave, r);
                    if (off != keep_epi_lds_off(wave, 0, l31, hh) + (uint32_t)(r * keep::ROW_STEP))
                        return fail("the row is not an additive constant", wp, wave, r);
                    const int u = (int)(off / 16);
                    // where the LDS-DMA would have read this unit from: the same pixel, the same half
                    const int row = keep::ROWS_PER_WAVE * wave + r + 1, col = l31 + 1;
                    const uint32_t want = (uint32_t)((row * wp + col) * 32 + hh * 16);
                    if (halo_unit_src(u, wp) != want) return fail("epilogue register on a foreign unit", wp, u, (int)want);
                    if (owner[u]) return fail("interior unit written twice", wp, u, owner[u]);
                    owner[u] = 1;
                    ++interior;
                }
    for (int i = 0; i < keep::RING_UNITS; ++i) {
        const int u = keep_ring_unit(i);
        if (u < 0 || u >= units) return fail("ring unit outside the image", wp, i, u);
        if (keep_ring_lds_off(i) != (uint32_t)(u * 16)) return fail("ring LDS offset", wp, i, u);
        if (keep_ring_src_off(i, wp) != halo_unit_src(u, wp)) return fail("ring source offset", wp, i, u);
        const int q = u >> 1, row = q / keep::HC, col = q % keep::HC;
        if (!(row == 0 || row == keep::HR - 1 || col == 0 || col == keep::HC - 1)) return fail("ring unit inside the tile", wp, i, u);
        if (owner[u]) return fail("ring unit taken twice or interior", wp, u, owner[u]);
        owner[u] = 2;
        ++ring;
    }
    int covered = 0;
    for (int u = 0; u < units; ++u) {
        if (!owner[u]) return fail("unit of a pixel q < 612 left unwritten", wp, u, 0);
        ++covered;
    }
    // the tail of the last 1 KB piece (never read) reads offset 0, as the LDS-DMA table has it
    for (int u = units; u < 20 * 64; ++u)
        if (halo_unit_src(u, wp) != 0) return fail("tail unit", wp, u, 0);
    std::printf("%d %d %d %d\n", wp, interior, ring, covered);
    return 0;
}

}  // namespace

int main() {
    for (int wp : {36, 54, 130, 8194})
        if (check(wp)) return 1;
    return 0;
}
