// Layout of a kept tile: what the persistent trunk kernel (trunk.hip) leaves in LDS across the
// phase-2 hand-off of a growth pair instead of reading it back from HBM.  No HIP dependency: the
// kernel and a host-only check (tests/test_trunk_keep_layout_cpu.py) include the same functions.
//
// The LDS halo image of one 16-channel chunk holds 18 x 34 pixels, pixel q = row * 34 + col, two
// 16-byte units each (8 channels); channel half c of pixel q sits at unit 2 q + (c ^ bit 3 of col).
// The LDS-DMA fills it unit by unit: unit u reads the in-plane byte offset halo_unit_src(u, wp)
// from the halo origin (wp = pixels per buffer row).
//  * Interior, 16 x 32 pixels = 1,024 units: exactly the packed 16-byte registers of the tile
//    epilogue.  Lane (l31, hh) of wave w holds, for its row r and each 16-channel plane, channel
//    half hh of output pixel (4 w + r, l31) = halo pixel (4 w + r + 1, l31 + 1).
//  * Ring, rows 0 and 17 and columns 0 and 33 of rows 1-16: 100 pixels = 200 units, written by
//    other workgroups (or padding).  Ring unit i (0..199) is taken by lane i of the workgroup.
#pragma once
#include <stdint.h>

namespace isr {

#if defined(__HIP__) || defined(__CUDACC__)
#define ISR_KEEP_HD __host__ __device__
#else
#define ISR_KEEP_HD
#endif

namespace keep {
constexpr int TH = 16, TW = 32;                        // tile (trunk_common.h tk::TH, tk::TW)
constexpr int HR = TH + 2, HC = TW + 2, HQ = HR * HC;  // halo pixels
constexpr int ROWS_PER_WAVE = 4;
constexpr int RING_PIXELS = 2 * HC + 2 * TH;           // 100
constexpr int RING_UNITS = 2 * RING_PIXELS;            // 200
constexpr int ROW_STEP = HC * 32;                      // LDS bytes from a halo row to the next
}  // namespace keep

// In-plane source byte offset (from the halo origin) of LDS unit u of the halo image; 0 for the
// never-read tail of the last 1 KB piece.
static inline ISR_KEEP_HD uint32_t halo_unit_src(int u, int wp) {
    const int q = u >> 1;
    if (q >= keep::HQ) return 0;
    const int row = q / keep::HC, col = q - row * keep::HC;
    const int cc = (u & 1) ^ ((col >> 3) & 1);
    return (uint32_t)((row * wp + col) * 32 + cc * 16);
}

// LDS byte offset, inside a slot's halo image, of the epilogue register of (wave, row r of the
// wave, lane l31 | hh << 5): the inverse of halo_unit_src for the tile's own pixels.  The row is an
// additive constant (r * ROW_STEP), so one per-lane base serves every row.
static inline ISR_KEEP_HD uint32_t keep_epi_lds_off(int wave, int r, int l31, int hh) {
    const int row = keep::ROWS_PER_WAVE * wave + r + 1, col = l31 + 1;
    const int q = row * keep::HC + col;
    return (uint32_t)((2 * q + (hh ^ ((col >> 3) & 1))) * 16);
}

// Ring unit i (0..RING_UNITS-1): its LDS unit index in the halo image.  Pixels in the order row 0,
// row 17, then (row, 0), (row, 33) for rows 1-16; two units per pixel.
static inline ISR_KEEP_HD int keep_ring_unit(int i) {
    const int p = i >> 1, s = i & 1;
    int row, col;
    if (p < keep::HC) {
        row = 0;
        col = p;
    } else if (p < 2 * keep::HC) {
        row = keep::HR - 1;
        col = p - keep::HC;
    } else {
        const int k = p - 2 * keep::HC;
        row = 1 + (k >> 1);
        col = (k & 1) ? keep::HC - 1 : 0;
    }
    return 2 * (row * keep::HC + col) + s;
}

static inline ISR_KEEP_HD uint32_t keep_ring_lds_off(int i) { return (uint32_t)(keep_ring_unit(i) * 16); }

// The ring unit's source offset, in the form the halo LDS-DMA uses for the same unit.
static inline ISR_KEEP_HD uint32_t keep_ring_src_off(int i, int wp) { return halo_unit_src(keep_ring_unit(i), wp); }

// What the kernel is told (bits).  The host switch ISR_TRUNK_KEEP, read once by the launch: 0 = OFF,
// 1 (default) = ON | BOUNDARY, 2 = ON alone (the A/B control of the boundary part).
enum : int {
    TRUNK_KEEP_OFF = 0,      // phase 2 stages its two chunks whole, at its own top
    TRUNK_KEEP_ON = 1,       // the interior and the weights stay in LDS; phase 2 fetches the ring only
    TRUNK_KEEP_BOUNDARY = 2  // also planes 0 and 1 of a final conv for the growth pair that follows it on
                             // the same tile (every RDB boundary when a workgroup owns one tile)
};

}  // namespace isr
