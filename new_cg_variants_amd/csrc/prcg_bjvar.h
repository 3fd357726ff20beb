// Variable-size point-block Jacobi (prcg_set_block_jacobi_var / prcg_build_block_jacobi_var): the HOST side of the device
// layout -- checking a partition, cutting it into tiles, laying the caller's packed blocks out for the kernels of
// prcg_blockjac.hip and reading them back.  Host-only, header-only, no HIP: O(nb) work from block_ptr, never the matrix.
//
// The layout (private to the library; prcg.h fixes only the packed host format and the arithmetic):
//   * the partition is cut greedily into TILES of consecutive whole blocks with at most 256 rows: a tile closes when the
//     next block does not fit, so no block straddles a workgroup; lane t of tile T owns row tile_row0[T] + t;
//   * a tile of largest block size L_T owns L_T LINES of 256 doubles, beginning at line tile_line0[T]: entry j of the row
//     of lane t sits at (tile_line0[T] + j) * 256 + t, so for a fixed j the 64 lanes of a wave read consecutive doubles;
//     a lane reads only j < m (its block's size); every other slot holds 0.0;
//   * per lane one CODE byte, tile-major (256 per tile): bits 0..2 the row's index a in its block, bits 3..5 m - 1, bit 7
//     set for a lane without a row; and one byte with the row's block index inside the tile (a tile has at most 256
//     blocks), which only the build kernel reads (its bad-block flag names a global block index);
//   * per tile four int64: tile_row0, tile_line0, tile_block0 (index of the tile's first block), L_T.
#ifndef PRCG_BJVAR_H
#define PRCG_BJVAR_H

#include <cstdint>
#include <vector>

namespace prcg {

constexpr int kBjvLanes = 256;          // lanes per workgroup = rows a tile can hold = doubles per line
constexpr int kBjvMaxSize = 8;          // largest block size
constexpr uint8_t kBjvDead = 0x80;      // code byte of a lane without a row
constexpr int kBjvTileWords = 4;        // int64 per tile in the device table

struct BjVarPlan {
    int64_t n = 0, nb = 0, ntiles = 0, lines = 0;          // lines: sum of L_T = doubles of the device layout / 256
    std::vector<int64_t> tiles;                            // ntiles x kBjvTileWords
    std::vector<uint8_t> code, bidx;                       // ntiles x 256 each
    int64_t doubles() const { return lines * kBjvLanes; }
};

// 0: a partition of n rows; 1: block_ptr[0] != 0; 2: block_ptr[nb] != n (or nb < 0); 3: a size outside 1..8, the first
// such block in *bad_block and its size in *bad_size
inline int bjvar_check(int64_t n, int64_t nb, const int64_t* ptr, int64_t* bad_block, int64_t* bad_size) {
    if (nb < 0) return 2;
    if (ptr[0] != 0) return 1;
    if (ptr[nb] != n) return 2;
    for (int64_t k = 0; k < nb; ++k) {
        const int64_t m = ptr[k + 1] - ptr[k];
        if (m < 1 || m > kBjvMaxSize) { *bad_block = k; *bad_size = m; return 3; }
    }
    return 0;
}

// the tiling of a CHECKED partition
inline void bjvar_plan(int64_t n, int64_t nb, const int64_t* ptr, BjVarPlan& P) {
    P = BjVarPlan{};
    P.n = n; P.nb = nb;
    int64_t k = 0;
    while (k < nb) {
        const int64_t row0 = ptr[k], block0 = k;
        int64_t L = 0;
        while (k < nb && ptr[k + 1] - row0 <= kBjvLanes) {
            const int64_t m = ptr[k + 1] - ptr[k];
            if (m > L) L = m;
            ++k;
        }
        P.tiles.push_back(row0); P.tiles.push_back(P.lines); P.tiles.push_back(block0); P.tiles.push_back(L);
        P.code.resize(P.code.size() + kBjvLanes, kBjvDead);
        P.bidx.resize(P.bidx.size() + kBjvLanes, 0);
        uint8_t* code = P.code.data() + P.ntiles * kBjvLanes;
        uint8_t* bidx = P.bidx.data() + P.ntiles * kBjvLanes;
        for (int64_t q = block0; q < k; ++q) {
            const int64_t m = ptr[q + 1] - ptr[q];
            for (int64_t a = 0; a < m; ++a) {
                const int64_t t = ptr[q] - row0 + a;
                code[t] = (uint8_t)(a | ((m - 1) << 3));
                bidx[t] = (uint8_t)(q - block0);
            }
        }
        P.lines += L;
        ++P.ntiles;
    }
}

// packed (block k as m_k x m_k row-major, no padding) -> device layout; laid: P.doubles() entries, every one written
inline void bjvar_lay(const BjVarPlan& P, const int64_t* ptr, const double* packed, double* laid) {
    for (int64_t q = 0; q < P.doubles(); ++q) laid[q] = 0.0;
    int64_t off = 0;
    for (int64_t T = 0; T < P.ntiles; ++T) {
        const int64_t* tw = P.tiles.data() + T * kBjvTileWords;
        const int64_t row0 = tw[0], line0 = tw[1], block0 = tw[2];
        const int64_t block1 = T + 1 < P.ntiles ? tw[kBjvTileWords + 2] : P.nb;
        for (int64_t k = block0; k < block1; ++k) {
            const int64_t m = ptr[k + 1] - ptr[k];
            for (int64_t a = 0; a < m; ++a)
                for (int64_t j = 0; j < m; ++j) laid[(line0 + j) * kBjvLanes + (ptr[k] - row0 + a)] = packed[off + a * m + j];
            off += m * m;
        }
    }
}

// the inverse of bjvar_lay; returns the number of packed doubles
inline int64_t bjvar_unlay(const BjVarPlan& P, const int64_t* ptr, const double* laid, double* packed) {
    int64_t off = 0;
    for (int64_t T = 0; T < P.ntiles; ++T) {
        const int64_t* tw = P.tiles.data() + T * kBjvTileWords;
        const int64_t row0 = tw[0], line0 = tw[1], block0 = tw[2];
        const int64_t block1 = T + 1 < P.ntiles ? tw[kBjvTileWords + 2] : P.nb;
        for (int64_t k = block0; k < block1; ++k) {
            const int64_t m = ptr[k + 1] - ptr[k];
            for (int64_t a = 0; a < m; ++a)
                for (int64_t j = 0; j < m; ++j) packed[off + a * m + j] = laid[(line0 + j) * kBjvLanes + (ptr[k] - row0 + a)];
            off += m * m;
        }
    }
    return off;
}

}  // namespace prcg
#endif  // PRCG_BJVAR_H
