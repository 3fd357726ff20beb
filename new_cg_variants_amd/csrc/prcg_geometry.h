// Geometry the host planner (prcg_plan.cpp) and the kernels (prcg_kernels.h and the .hip files) must agree on: the tile
// descriptors the kernels read and the constants that size them.  ONE definition of each, no HIP header -- the planner
// is also built with a plain host compiler (tools/run_plan_asan.py, tools/plan_operator_check.cpp).
#pragma once
#include <stdint.h>

namespace prcg {

// ---- CSR-adaptive tiles ------------------------------------------------------------------------
// A tile is a run of consecutive rows handled by ONE wavefront: its nonzeros are
// streamed with 16-byte loads, the products staged in that wave's LDS slice, and each
// row reduced sequentially (left to right, as scipy's csr_matvec does) by one lane.
constexpr int kDefaultTileSteps = 2;                // 256-nnz steps per tile (1, 2 or 4)
inline int tile_cap_nnz(int steps) { return 256 * steps - 3; }   // -3: the stream starts 16-B aligned
constexpr int kTileCapRows = 256;
struct alignas(16) Tile { int row_begin, row_end, nnz_begin, nnz_end; };
static_assert(sizeof(Tile) == 16, "the kernels read a tile descriptor as one int4");
constexpr int kDictMax = 64;   // value dictionary of a tile: one entry per lane
// spare entries behind every gather-source vector: the largest tile-relative column offset (16 bit)
// added to a valid column of the tile never leaves the allocation
constexpr int kGatherPad = 65536;
// experiment knob of the tile kernels (PRCG_GRID_PER_CU)
struct TileKnobs { int per_cu = 0; };

// ---- window tiles (row-per-lane kernels, prcg_win.hip; planned by plan_window_tiles) ----------------
constexpr int kWinSlots = 1024;                 // nonzeros of one window tile that fit the wave's LDS slice
constexpr int kWinCapNnz = kWinSlots - 15;      // the stream starts at a multiple of 16 nonzeros
constexpr int kWinDictMax = 256;
constexpr int kWinMaxPages = 12;
struct alignas(16) WTile {
    int rb, re, lo, hi;                  // rows [rb,re), nonzeros [lo,hi)
    int geo, maxlen, vd_first, vd_count;      // geo = pages in use | (window index of row rb) << 8; longest row;
                                         // value dictionary {first entry, count}
    int page_col[kWinMaxPages];          // first column of each page
    // where the kernel reads the tile's encoded streams (share_window_streams): 16-aligned start of the
    // window-index image / of the value-index image (elements), start of the relative row pointers
    int src_c, src_v, src_r, spare;      // spare: image id (share_window_streams), equal for tiles that read identical streams
};
static_assert(sizeof(WTile) == 96, "the kernels read a window tile descriptor as six int4");

// pattern tiles (prcg_plan.h: plan_window_patterns): constant-coefficient stencils without index streams
constexpr int kPatSlots = 16;
constexpr int kPatValues = 4;
struct alignas(8) PatRec {
    int nslots;                 // U
    unsigned vsel;              // 2 bits per slot: which of val[] the slot's value is
    short cb[kPatSlots];        // slot u sits at window index lane + cb[u]  (may be negative for lanes without the slot)
    double val[kPatValues];     // the caller's doubles, bit for bit
};
static_assert(sizeof(PatRec) == 72, "the kernels read a pattern record with scalar loads");

// geometry id of a class planned with rows_per_tile (64 | 128) whose tiles need at most most_pages
// pages: 0 = 64 rows / 2 pages / 8-bit indices, 1 = 64 / 4 / 8-bit, 2 = 128 / 8 / 16-bit, 3 = 128 / 12 / 16-bit,
// 4 = 64 / 8 / 16-bit (3-D stencils in 64-row tiles: images repeat with the period of a grid plane)
// 5 = 64 rows / 6 pages / PATTERN tiles (constant-coefficient stencils, no index streams; chosen by plan_operator when every
//     tile qualifies, prcg_plan.h: plan_window_patterns)
constexpr int kWinPatGeom = 5, kWinPatPages = 6;
inline int win_geometry(int rows_per_tile, int most_pages) {
    if (rows_per_tile == 64) return most_pages <= 2 ? 0 : (most_pages <= 4 ? 1 : (most_pages <= 8 ? 4 : -1));
    if (rows_per_tile == 128) return most_pages <= 8 ? 2 : (most_pages <= 12 ? 3 : -1);
    return -1;
}
inline int win_max_pages(int rows_per_tile) { return rows_per_tile == 64 ? 8 : 12; }

}  // namespace prcg
