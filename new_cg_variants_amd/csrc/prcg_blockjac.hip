// gfx950 (MI355X / CDNA4): point-block Jacobi, out = blockdiag(B_0 .. B_{nb-1}) v with one uniform block size bs in 1..8
// (prcg_set_block_jacobi; PETSc's -pc_type pbjacobi -- the reference has only the Jacobi lambda, figure_gen.py:43).
//
// Arithmetic (prcg.h): row i = k*bs + a computes  acc = B[k][a][0] * v[k*bs];  acc = acc + B[k][a][j] * v[k*bs + j]
// for ascending j -- every product and every sum rounded (-ffp-contract=off), so the result has the bits of the same
// loop written with NumPy multiplies and adds on the host.  A short last block (n not a multiple of bs) uses its
// leading m x m part only; nothing at or beyond row n is read or written.
//
// The kernel is bandwidth bound: per row it must read the row's bs block entries and one entry of v and write one
// entry, (bs + 2) * 8 bytes.  Row per lane, wave64, 256 lanes per workgroup:
//
//   * a workgroup owns a TILE of TR = 256 - 256 % bs consecutive rows (255 at bs = 3), a whole number of blocks, so no
//     block straddles two workgroups; lanes TR..255 idle (at most 6 of 256);
//   * the caller's row-major nb x bs x bs array would make lane t read address (t * bs + j) * 8 for a fixed j: a
//     stride of bs doubles, bs times the cache lines per instruction.  The blocks are therefore RE-LAID ONCE AT UPLOAD
//     (block_jacobi_layout, below): entry j of the row of lane t of tile T sits at ((T * bs + j) * 256 + t), so that
//     for a fixed j the 64 lanes of a wave read 64 consecutive doubles (512 B, aligned: the tile stride is 256
//     entries, not TR, which costs 256 % bs / 256 of padding -- 0.4 % at bs = 3);
//   * every lane loads ITS entry of v (coalesced; stride 2 when the vector is one column of a pair array) and parks it
//     in LDS; after one barrier the lane reads its block's bs entries from there (lanes of one row-block read the
//     same LDS address: a broadcast) -- one global load of v per row instead of bs;
//   * the pair form does both columns of the pipelined loop's interleaved [w u] array in one launch: one 16-byte load
//     per row brings (w_i, u_i), the block entries are read once and used for both: (bs + 4) * 8 bytes per row
//     instead of 2 * (bs + 2) * 8.
#include <hip/hip_runtime.h>

#include "prcg_kernels.h"
#include "prcg_device.hpp"

namespace prcg {
namespace {

constexpr int kBjBlock = 256;    // lanes per workgroup = entries per (tile, j) line of the device layout
static_assert(kBjBlock == kBlock, "block_reduce_store sums the four waves of a 256-lane workgroup");

typedef double d2_t __attribute__((ext_vector_type(2)));

template <int BS>
__global__ __launch_bounds__(kBjBlock) void k_block_jacobi(double* __restrict__ dst, int ds, const double* __restrict__ src, int ss,
                                                           int64_t n, const double* __restrict__ blk) {
    constexpr int TR = (kBjBlock / BS) * BS;
    __shared__ double sv[kBjBlock];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * TR;
    const int64_t i = row0 + t;
    const bool live = t < TR && i < n;
    if (live) sv[t] = src[i * ss];
    __syncthreads();
    if (!live) return;
    const int c0 = t - t % BS;                            // first lane of this row's block
    const int64_t cols = n - (row0 + c0);                 // columns the block really has (>= BS except in a short last block)
    const double* bp = blk + ((int64_t)blockIdx.x * BS) * kBjBlock + t;
    double b[BS];
#pragma unroll
    for (int j = 0; j < BS; ++j) b[j] = bp[(int64_t)j * kBjBlock];
    double acc = b[0] * sv[c0];
#pragma unroll
    for (int j = 1; j < BS; ++j)
        if (j < cols) acc = acc + b[j] * sv[c0 + j];
    dst[i * ds] = acc;
}

// both columns of the interleaved [w u] array: wt = M^-1 w (mask bit 0), ut = M^-1 u (mask bit 1)
template <int BS>
__device__ __forceinline__ void block_jacobi_pair_body(double* __restrict__ wt, double* __restrict__ ut, const d2_t* __restrict__ wu,
                                                       int64_t n, const double* __restrict__ blk, int mask) {
    constexpr int TR = (kBjBlock / BS) * BS;
    __shared__ d2_t sv[kBjBlock];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * TR;
    const int64_t i = row0 + t;
    const bool live = t < TR && i < n;
    if (live) sv[t] = wu[i];
    __syncthreads();
    if (!live) return;
    const int c0 = t - t % BS;
    const int64_t cols = n - (row0 + c0);
    const double* bp = blk + ((int64_t)blockIdx.x * BS) * kBjBlock + t;
    double b[BS];
#pragma unroll
    for (int j = 0; j < BS; ++j) b[j] = bp[(int64_t)j * kBjBlock];
    d2_t v = sv[c0];
    double aw = b[0] * v.x, au = b[0] * v.y;
#pragma unroll
    for (int j = 1; j < BS; ++j)
        if (j < cols) {
            v = sv[c0 + j];
            aw = aw + b[j] * v.x;
            au = au + b[j] * v.y;
        }
    if (mask & 1) wt[i] = aw;
    if (mask & 2) ut[i] = au;
}
template <int BS>
__global__ __launch_bounds__(kBjBlock) void k_block_jacobi_pair(double* __restrict__ wt, double* __restrict__ ut, const d2_t* __restrict__ wu,
                                                                int64_t n, const double* __restrict__ blk, int mask) {
    block_jacobi_pair_body<BS>(wt, ut, wu, n, blk, mask);
}
// Head of the pair launch of iteration k of a session that stops (ProductStop, prcg_kernels.h; prcg_set_stop_block_jacobi): true if
// the session stopped BEFORE iteration k -- the pair launch of the stop iteration itself belongs to that iteration's state.  The
// word was complete before the launch began (kernel boundary), every wave reads the same value: a workgroup leaves as a whole on a
// scalar branch, before anything is loaded or stored and before the kernel's barrier.
__device__ __forceinline__ bool pair_stopped(const ProductStop& stop) {
    const int at = __builtin_amdgcn_readfirstlane(stop.word[0]);
    return at >= 0 && at < stop.k;
}
// ... the stop form: the same statements behind that head
template <int BS>
__global__ __launch_bounds__(kBjBlock) void k_block_jacobi_pair_stop(double* __restrict__ wt, double* __restrict__ ut, const d2_t* __restrict__ wu,
                                                                     int64_t n, const double* __restrict__ blk, int mask, ProductStop stop) {
    if (pair_stopped(stop)) return;
    block_jacobi_pair_body<BS>(wt, ut, wu, n, blk, mask);
}

inline int bj_grid(int64_t n, int bs) {
    const int64_t tr = (kBjBlock / bs) * bs;
    return (int)((n + tr - 1) / tr);
}

template <int BS>
void launch_one(hipStream_t st, double* dst, int ds, const double* src, int ss, int64_t n, const double* blk) {
    hipLaunchKernelGGL(k_block_jacobi<BS>, dim3(bj_grid(n, BS)), dim3(kBjBlock), 0, st, dst, ds, src, ss, n, blk);
}
template <int BS>
void launch_two(hipStream_t st, double* wt, double* ut, const double* wu, int64_t n, const double* blk, int mask, const StopAt& stop) {
    if (stop)
        hipLaunchKernelGGL(k_block_jacobi_pair_stop<BS>, dim3(bj_grid(n, BS)), dim3(kBjBlock), 0, st, wt, ut, reinterpret_cast<const d2_t*>(wu), n,
                           blk, mask, stop.skips());
    else
        hipLaunchKernelGGL(k_block_jacobi_pair<BS>, dim3(bj_grid(n, BS)), dim3(kBjBlock), 0, st, wt, ut, reinterpret_cast<const d2_t*>(wu), n,
                           blk, mask);
}

// ---- the device build (prcg_build_block_jacobi): gather the diagonal blocks from the caller-order CSR arrays, invert them, store
// them in the layout above -- one pass over the operator, no host re-lay, no upload.  The arithmetic is the contract of prcg.h
// (cg_variants.invert_blocks restates it): per row g[c] = g[c] + val[q] over the row's nonzeros in CSR order, then Gauss-Jordan on
// [M | E] without pivoting, a division per entry of the pivot row, a product and a difference per entry of every other row.
//   * lane per row, the tiling of k_block_jacobi: lane t of tile T owns row T * TR + t and keeps its row of [M | E], 2 * BS doubles;
//   * the row walk reads the column first and loads the value only on a match (about BS of a row's entries match);
//   * at step c the lane with a == c scales its row and parks it in LDS for its block; after ONE barrier the other lanes of the
//     block eliminate (the parking area is double buffered by the step's parity, so the next pivot row is written while slow lanes
//     still read this one).  Blocks straddle waves (TR = 255 at bs = 3): hence LDS and the workgroup barrier, not shuffles;
//   * the rows a short last block lacks are played by their lanes as identity rows, so the block runs the whole loop as the host
//     restatement does; they store 0 like every lane without a row, as block_jacobi_layout does;
//   * a bad block (a pivot zero or not finite at its step, an entry of E not finite) takes the minimum of its index into *first_bad.
template <int BS>
__global__ __launch_bounds__(kBjBlock) void k_block_jacobi_build(double* __restrict__ blk, int64_t n, const int* __restrict__ indptr,
                                                                 const int* __restrict__ col, const double* __restrict__ val,
                                                                 long long* __restrict__ first_bad) {
    constexpr int TR = (kBjBlock / BS) * BS;
    __shared__ double park[2][kBjBlock / BS][2 * BS];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * TR;
    const int64_t i = row0 + t;
    const int a = t % BS, lb = t / BS;
    const int64_t kb = i - a;                             // first row of this row's block (row0 is a multiple of BS)
    const bool live = t < TR && i < n;                    // the lane has a row
    const bool member = t < TR && kb < n;                 // ... or plays an identity row of a short last block
    double M[BS], E[BS];
#pragma unroll
    for (int j = 0; j < BS; ++j) { M[j] = (!live && j == a) ? 1.0 : 0.0; E[j] = j == a ? 1.0 : 0.0; }
    if (live) {
        const int q1 = indptr[i + 1];
        const int c0 = (int)kb;
        for (int q = indptr[i]; q < q1; ++q) {
            const int c = col[q] - c0;
            if (c >= 0 && c < BS) {
                const double v = val[q];
#pragma unroll
                for (int j = 0; j < BS; ++j)
                    if (c == j) M[j] = M[j] + v;
            }
        }
    }
    bool bad = false;
#pragma unroll
    for (int c = 0; c < BS; ++c) {
        double* pr = park[c & 1][lb];
        if (member && a == c) {
            const double p = M[c];
            bad = bad || p == 0.0 || !(p - p == 0.0);     // zero, infinite or NaN
#pragma unroll
            for (int j = 0; j < BS; ++j) { M[j] = M[j] / p; E[j] = E[j] / p; pr[j] = M[j]; pr[BS + j] = E[j]; }
        }
        __syncthreads();
        if (member && a != c) {
            const double f = M[c];
#pragma unroll
            for (int j = 0; j < BS; ++j) { M[j] = M[j] - f * pr[j]; E[j] = E[j] - f * pr[BS + j]; }
        }
    }
    if (member) {
#pragma unroll
        for (int j = 0; j < BS; ++j) bad = bad || !(E[j] - E[j] == 0.0);
        if (bad) atomicMin(first_bad, (long long)(kb / BS));
    }
    double* out = blk + ((int64_t)blockIdx.x * BS) * kBjBlock + t;
#pragma unroll
    for (int j = 0; j < BS; ++j) out[(int64_t)j * kBjBlock] = live ? E[j] : 0.0;
}

template <int BS>
void launch_build(hipStream_t st, double* blk, int64_t n, const int* indptr, const int* col, const double* val, long long* first_bad) {
    hipLaunchKernelGGL(k_block_jacobi_build<BS>, dim3(bj_grid(n, BS)), dim3(kBjBlock), 0, st, blk, n, indptr, col, val, first_bad);
}

// ---- variable block sizes (prcg_set_block_jacobi_var / prcg_build_block_jacobi_var; PETSc's -pc_type vpbjacobi): block k owns
// rows block_ptr[k] .. block_ptr[k+1]-1, every size in 1..8.  The arithmetic is word for word that of the kernels above, the loop
// over j bounded by the row's own size m instead of a template parameter.  The device layout is prcg_bjvar.h's: a TILE is a run of
// consecutive whole blocks with at most 256 rows (no block straddles a workgroup); the tile table gives a workgroup its first
// row and its first LINE, a code byte gives a lane its index a in its block and the block's size m (one coalesced byte load).
// Coalescing: entry j of the row of lane t of tile T sits at (line0[T] + j) * 256 + t, so for a fixed j the lanes of a wave read
// consecutive doubles, as above; a lane loads only j < m, so in a mix of sizes the lines j >= 3, say, are touched by the runs of
// lanes whose blocks are that wide (a run of six lanes is 48 of a 64-byte sector).  A row moves (m + 2) * 8 + 1 useful bytes.
// The eight loads are unrolled and predicated (j < m), not a loop with a data-dependent trip count: all are in flight together.
// LDS: a lane reads sv[c0 + j] for j < m only, i.e. inside its own block's lanes; the arrays carry 8 spare entries so that even
// a load hoisted above its predicate stays inside them.
constexpr int kBjvPad = 8;
constexpr int kBjvDeadBit = 0x80;     // prcg_bjvar.h: kBjvDead

__global__ __launch_bounds__(kBjBlock) void k_block_jacobi_var(double* __restrict__ dst, int ds, const double* __restrict__ src, int ss,
                                                               const long long* __restrict__ tiles, const unsigned char* __restrict__ code,
                                                               const double* __restrict__ blk) {
    __shared__ double sv[kBjBlock + kBjvPad];
    const int t = threadIdx.x;
    const long long* tw = tiles + (int64_t)blockIdx.x * 4;
    const int64_t i = tw[0] + t;
    const int cd = code[(int64_t)blockIdx.x * kBjBlock + t];
    const bool live = !(cd & kBjvDeadBit);
    if (live) sv[t] = src[i * ss];
    __syncthreads();
    if (!live) return;
    const int a = cd & 7, m = ((cd >> 3) & 7) + 1;
    const int c0 = t - a;                                 // first lane of this row's block
    const double* bp = blk + tw[1] * kBjBlock + t;
    double b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = j < m ? bp[(int64_t)j * kBjBlock] : 0.0;
    double acc = b[0] * sv[c0];
#pragma unroll
    for (int j = 1; j < 8; ++j)
        if (j < m) acc = acc + b[j] * sv[c0 + j];
    dst[i * ds] = acc;
}

__device__ __forceinline__ void block_jacobi_var_pair_body(double* __restrict__ wt, double* __restrict__ ut, const d2_t* __restrict__ wu,
                                                           const long long* __restrict__ tiles, const unsigned char* __restrict__ code,
                                                           const double* __restrict__ blk, int mask) {
    __shared__ d2_t sv[kBjBlock + kBjvPad];
    const int t = threadIdx.x;
    const long long* tw = tiles + (int64_t)blockIdx.x * 4;
    const int64_t i = tw[0] + t;
    const int cd = code[(int64_t)blockIdx.x * kBjBlock + t];
    const bool live = !(cd & kBjvDeadBit);
    if (live) sv[t] = wu[i];
    __syncthreads();
    if (!live) return;
    const int a = cd & 7, m = ((cd >> 3) & 7) + 1;
    const int c0 = t - a;
    const double* bp = blk + tw[1] * kBjBlock + t;
    double b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = j < m ? bp[(int64_t)j * kBjBlock] : 0.0;
    d2_t v = sv[c0];
    double aw = b[0] * v.x, au = b[0] * v.y;
#pragma unroll
    for (int j = 1; j < 8; ++j)
        if (j < m) {
            v = sv[c0 + j];
            aw = aw + b[j] * v.x;
            au = au + b[j] * v.y;
        }
    if (mask & 1) wt[i] = aw;
    if (mask & 2) ut[i] = au;
}
__global__ __launch_bounds__(kBjBlock) void k_block_jacobi_var_pair(double* __restrict__ wt, double* __restrict__ ut, const d2_t* __restrict__ wu,
                                                                    const long long* __restrict__ tiles, const unsigned char* __restrict__ code,
                                                                    const double* __restrict__ blk, int mask) {
    block_jacobi_var_pair_body(wt, ut, wu, tiles, code, blk, mask);
}
// ... the stop form (pair_stopped above): the same statements behind the head
__global__ __launch_bounds__(kBjBlock) void k_block_jacobi_var_pair_stop(double* __restrict__ wt, double* __restrict__ ut, const d2_t* __restrict__ wu,
                                                                         const long long* __restrict__ tiles, const unsigned char* __restrict__ code,
                                                                         const double* __restrict__ blk, int mask, ProductStop stop) {
    if (pair_stopped(stop)) return;
    block_jacobi_var_pair_body(wt, ut, wu, tiles, code, blk, mask);
}

// the device build for a partition: k_block_jacobi_build's scheme, lane per row, with the row's own m.
//   * the row walk needs no block_ptr: the row's block owns columns [row0 + c0, row0 + c0 + m);
//   * the steps are bounded by L, the tile's largest size (uniform over the workgroup, so every lane meets every barrier); a
//     lane takes part in step c only if c < m, and touches only entries j < m of its rows of M and E;
//   * the pivot row is parked in the slots of the block's own lanes: pm / pe[parity][c0 + j], j < m (8 KB whatever the sizes);
//   * every slot of the tile's L lines is written: E[j] for j < m, 0.0 elsewhere (the layout's "slots never loaded hold 0.0").
__global__ __launch_bounds__(kBjBlock) void k_block_jacobi_var_build(double* __restrict__ blk, const long long* __restrict__ tiles,
                                                                     const unsigned char* __restrict__ code, const unsigned char* __restrict__ bidx,
                                                                     const int* __restrict__ indptr, const int* __restrict__ col,
                                                                     const double* __restrict__ val, long long* __restrict__ first_bad) {
    __shared__ double pm[2][kBjBlock + kBjvPad], pe[2][kBjBlock + kBjvPad];
    const int t = threadIdx.x;
    const long long* tw = tiles + (int64_t)blockIdx.x * 4;
    const int64_t row0 = tw[0], i = row0 + t;
    const int L = (int)tw[3];
    const int cd = code[(int64_t)blockIdx.x * kBjBlock + t];
    const bool live = !(cd & kBjvDeadBit);
    const int a = cd & 7, m = live ? ((cd >> 3) & 7) + 1 : 0;
    const int c0 = t - a;
    double M[8], E[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { M[j] = 0.0; E[j] = j == a ? 1.0 : 0.0; }
    if (live) {
        const int q1 = indptr[i + 1];
        const int64_t cb = row0 + c0;                     // first column of the row's block
        for (int q = indptr[i]; q < q1; ++q) {
            const int64_t c = (int64_t)col[q] - cb;
            if (c >= 0 && c < m) {
                const double v = val[q];
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (c == j) M[j] = M[j] + v;
            }
        }
    }
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (c < L) {                                      // uniform over the workgroup
            double* qm = pm[c & 1] + c0;
            double* qe = pe[c & 1] + c0;
            if (c < m && a == c) {
                const double p = M[c];
                bad = bad || p == 0.0 || !(p - p == 0.0);     // zero, infinite or NaN
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (j < m) { M[j] = M[j] / p; E[j] = E[j] / p; qm[j] = M[j]; qe[j] = E[j]; }
            }
            __syncthreads();
            if (c < m && a != c) {
                const double f = M[c];
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (j < m) { M[j] = M[j] - f * qm[j]; E[j] = E[j] - f * qe[j]; }
            }
        }
    }
    if (live) {
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < m) bad = bad || !(E[j] - E[j] == 0.0);
        if (bad) atomicMin(first_bad, tw[2] + (long long)bidx[(int64_t)blockIdx.x * kBjBlock + t]);
    }
    double* out = blk + tw[1] * kBjBlock + t;
#pragma unroll
    for (int j = 0; j < 8; ++j)
        if (j < L) out[(int64_t)j * kBjBlock] = j < m ? E[j] : 0.0;
}

// ---- M^-1 on an interleaved n x 2 array WITH the inner products that need the result, in one launch: the block-Jacobi sessions
// with two or four right-hand sides (prcg_solve_begin_multi_block_jacobi).  The apply is k_block_jacobi_pair's (k_block_jacobi_var_pair's):
// one 16-byte load per row, the pair parked in LDS, one barrier, the block's entries read from LDS as a broadcast, the row of the
// inverse loaded with coalesced reads and used for BOTH columns; one 16-byte store of (z_0, z_1).  Two modes:
//   kBjDotsNu   z = M^-1 r -> r~;  partials of nu_c = r_c.z_c and rr_c = r_c.r_c                       (m + 4) * 8 useful bytes per row
//   kBjDotsPr   z = M^-1 s -> s~;  partials of mu_c = p_c.s_c, dl_c = r_c.z_c, gm_c = z_c.s_c          (m + 8) * 8
// Sums: ONE partial row per tile.  Lane t holds the products of row tile_row0 + t -- a lane WITHOUT a row holds +0.0 and stays to
// the end: the block reduction has a barrier of its own, so nobody returns after the first one -- xor butterfly per wave, waves
// 0..3 in order (block_reduce_store / block_reduce_store2), the tile partials in tile order by the final tree.  The tiles are a
// function of n and the partition alone.  The uniform tiles of 256 - 256 % bs rows are the greedy tiles of bjvar_plan on the uniform
// partition, and both forms then sum in the same tree -- with ONE exception: where a short last block fits into the 256 % bs lanes
// a full tile leaves idle (n mod (256 - 256 % bs) in 1 .. 256 % bs) the greedy tiling takes it into the last full tile while the
// uniform kernel gives it a tile of its own; for such n the two forms have different trees and need not give equal bits.
// Each column has its own accumulators; no branch on a value.
// Partial rows: NU with part1 == nullptr writes [nu_0 rr_0 nu_1 rr_1] to slots 3..6 of part0 (the Hestenes-Stiefel scalar row);
// otherwise column c's sums go to part[c] in the single-session slots (NU: 3, 4; PR: 0, 1, 2).
template <int MODE>
__device__ __forceinline__ void bj_dots_finish(const BjDotsArgs& a, int64_t i, bool live, d2_t own, d2_t z, d2_t pv, d2_t rv) {
    if (live) reinterpret_cast<d2_t*>(a.z)[i] = z;
    if constexpr (MODE == kBjDotsNu) {
        double acc[4] = {0.0, 0.0, 0.0, 0.0};                   // nu_0, rr_0, nu_1, rr_1
        if (live) { acc[0] = own.x * z.x; acc[1] = own.x * own.x; acc[2] = own.y * z.y; acc[3] = own.y * own.y; }
        if (a.part1) block_reduce_store2<2>(acc, a.part0, a.part1, kPr2Nu);       // (uniform over the launch)
        else block_reduce_store<4>(acc, a.part0, kHs2Nu);
    } else {
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};         // mu_0, dl_0, gm_0, mu_1, dl_1, gm_1
        if (live) {
            acc[0] = pv.x * own.x; acc[1] = rv.x * z.x; acc[2] = z.x * own.x;
            acc[3] = pv.y * own.y; acc[4] = rv.y * z.y; acc[5] = z.y * own.y;
        }
        block_reduce_store2<3>(acc, a.part0, a.part1, kPr2Mu);
    }
}

template <int BS, int MODE>
__global__ __launch_bounds__(kBjBlock) void k_block_jacobi_dots(BjDotsArgs a, const double* __restrict__ blk) {
    constexpr int TR = (kBjBlock / BS) * BS;
    __shared__ d2_t sv[kBjBlock];
    const int t = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * TR;
    const int64_t i = row0 + t;
    const bool live = t < TR && i < a.n;
    d2_t own = {0.0, 0.0}, pv = {0.0, 0.0}, rv = {0.0, 0.0}, z = {0.0, 0.0};
    double b[BS];
#pragma unroll
    for (int j = 0; j < BS; ++j) b[j] = 0.0;
    if (live) {
        own = reinterpret_cast<const d2_t*>(a.v)[i];
        sv[t] = own;
        const double* bp = blk + ((int64_t)blockIdx.x * BS) * kBjBlock + t;
#pragma unroll
        for (int j = 0; j < BS; ++j) b[j] = bp[(int64_t)j * kBjBlock];
        if constexpr (MODE == kBjDotsPr) { pv = reinterpret_cast<const d2_t*>(a.p)[i]; rv = reinterpret_cast<const d2_t*>(a.r)[i]; }
    }
    __syncthreads();
    if (live) {
        const int c0 = t - t % BS;                            // first lane of this row's block
        const int64_t cols = a.n - (row0 + c0);               // columns the block really has (>= BS except in a short last block)
        d2_t v = sv[c0];
        z.x = b[0] * v.x; z.y = b[0] * v.y;
#pragma unroll
        for (int j = 1; j < BS; ++j)
            if (j < cols) {
                v = sv[c0 + j];
                z.x = z.x + b[j] * v.x;
                z.y = z.y + b[j] * v.y;
            }
    }
    bj_dots_finish<MODE>(a, i, live, own, z, pv, rv);
}

template <int MODE>
__global__ __launch_bounds__(kBjBlock) void k_block_jacobi_var_dots(BjDotsArgs a, const long long* __restrict__ tiles,
                                                                    const unsigned char* __restrict__ code, const double* __restrict__ blk) {
    __shared__ d2_t sv[kBjBlock + kBjvPad];
    const int t = threadIdx.x;
    const long long* tw = tiles + (int64_t)blockIdx.x * 4;
    const int64_t i = tw[0] + t;
    const int cd = code[(int64_t)blockIdx.x * kBjBlock + t];
    const bool live = !(cd & kBjvDeadBit);
    const int aa = cd & 7, m = ((cd >> 3) & 7) + 1;
    d2_t own = {0.0, 0.0}, pv = {0.0, 0.0}, rv = {0.0, 0.0}, z = {0.0, 0.0};
    double b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) b[j] = 0.0;
    if (live) {
        own = reinterpret_cast<const d2_t*>(a.v)[i];
        sv[t] = own;
        const double* bp = blk + tw[1] * kBjBlock + t;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < m) b[j] = bp[(int64_t)j * kBjBlock];
        if constexpr (MODE == kBjDotsPr) { pv = reinterpret_cast<const d2_t*>(a.p)[i]; rv = reinterpret_cast<const d2_t*>(a.r)[i]; }
    }
    __syncthreads();
    if (live) {
        const int c0 = t - aa;                                // first lane of this row's block
        d2_t v = sv[c0];
        z.x = b[0] * v.x; z.y = b[0] * v.y;
#pragma unroll
        for (int j = 1; j < 8; ++j)
            if (j < m) {
                v = sv[c0 + j];
                z.x = z.x + b[j] * v.x;
                z.y = z.y + b[j] * v.y;
            }
    }
    bj_dots_finish<MODE>(a, i, live, own, z, pv, rv);
}

template <int BS>
void launch_dots(hipStream_t st, int mode, const BjDotsArgs& a, const double* blk) {
    const dim3 grid(bj_grid(a.n, BS)), block(kBjBlock);
    if (mode == kBjDotsNu) hipLaunchKernelGGL((k_block_jacobi_dots<BS, kBjDotsNu>), grid, block, 0, st, a, blk);
    else hipLaunchKernelGGL((k_block_jacobi_dots<BS, kBjDotsPr>), grid, block, 0, st, a, blk);
}

}  // namespace

int64_t block_jacobi_tiles(int64_t n, int bs) { return (bs < 1 || bs > 8 || n <= 0) ? 0 : bj_grid(n, bs); }

int launch_block_jacobi_dots(hipStream_t st, int mode, const BjDotsArgs& a, int bs, const double* blocks) {
    if (a.n <= 0 || (mode != kBjDotsNu && mode != kBjDotsPr)) return -1;
    switch (bs) {
    case 1: launch_dots<1>(st, mode, a, blocks); break;
    case 2: launch_dots<2>(st, mode, a, blocks); break;
    case 3: launch_dots<3>(st, mode, a, blocks); break;
    case 4: launch_dots<4>(st, mode, a, blocks); break;
    case 5: launch_dots<5>(st, mode, a, blocks); break;
    case 6: launch_dots<6>(st, mode, a, blocks); break;
    case 7: launch_dots<7>(st, mode, a, blocks); break;
    case 8: launch_dots<8>(st, mode, a, blocks); break;
    default: return -1;
    }
    return hipGetLastError() == hipSuccess ? bj_grid(a.n, bs) : -1;
}

int launch_block_jacobi_var_dots(hipStream_t st, int mode, const BjDotsArgs& a, int64_t ntiles, const long long* tiles,
                                 const unsigned char* code, const double* blocks) {
    if (ntiles <= 0 || (mode != kBjDotsNu && mode != kBjDotsPr)) return -1;
    const dim3 grid((unsigned)ntiles), block(kBjBlock);
    if (mode == kBjDotsNu) hipLaunchKernelGGL(k_block_jacobi_var_dots<kBjDotsNu>, grid, block, 0, st, a, tiles, code, blocks);
    else hipLaunchKernelGGL(k_block_jacobi_var_dots<kBjDotsPr>, grid, block, 0, st, a, tiles, code, blocks);
    return hipGetLastError() == hipSuccess ? (int)ntiles : -1;
}

int launch_block_jacobi_var(hipStream_t st, double* dst, int dstride, const double* src, int sstride, int64_t ntiles, const long long* tiles,
                            const unsigned char* code, const double* blocks) {
    if (ntiles <= 0) return 0;
    hipLaunchKernelGGL(k_block_jacobi_var, dim3((unsigned)ntiles), dim3(kBjBlock), 0, st, dst, dstride, src, sstride, tiles, code, blocks);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_block_jacobi_var_pair(hipStream_t st, double* wt, double* ut, const double* wu, int64_t ntiles, const long long* tiles,
                                 const unsigned char* code, const double* blocks, int mask, const StopAt& stop) {
    if (ntiles <= 0) return 0;
    if (stop)
        hipLaunchKernelGGL(k_block_jacobi_var_pair_stop, dim3((unsigned)ntiles), dim3(kBjBlock), 0, st, wt, ut, reinterpret_cast<const d2_t*>(wu), tiles,
                           code, blocks, mask, stop.skips());
    else
        hipLaunchKernelGGL(k_block_jacobi_var_pair, dim3((unsigned)ntiles), dim3(kBjBlock), 0, st, wt, ut, reinterpret_cast<const d2_t*>(wu), tiles,
                           code, blocks, mask);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_block_jacobi_var_build(hipStream_t st, double* blocks, int64_t ntiles, const long long* tiles, const unsigned char* code,
                                  const unsigned char* bidx, const int* indptr, const int* col, const double* val, long long* first_bad) {
    if (ntiles <= 0) return 0;
    hipLaunchKernelGGL(k_block_jacobi_var_build, dim3((unsigned)ntiles), dim3(kBjBlock), 0, st, blocks, tiles, code, bidx, indptr, col, val,
                       first_bad);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int64_t block_jacobi_layout(int64_t n, int bs, const double* inv_blocks, double* out) {
    if (n < 0 || bs < 1 || bs > 8) return -1;
    const int64_t tr = (kBjBlock / bs) * bs;
    const int64_t ntiles = (n + tr - 1) / tr;
    const int64_t total = ntiles * bs * kBjBlock;
    if (!out) return total;
    for (int64_t T = 0; T < ntiles; ++T)
        for (int j = 0; j < bs; ++j) {
            double* line = out + (T * bs + j) * kBjBlock;
            for (int t = 0; t < kBjBlock; ++t) {
                const int64_t i = T * tr + t;             // row i = block i / bs, row i % bs of it
                line[t] = (t < tr && i < n) ? inv_blocks[i * bs + j] : 0.0;
            }
        }
    return total;
}

int64_t block_jacobi_unlay(int64_t n, int bs, const double* laid, double* inv_blocks) {
    if (n < 0 || bs < 1 || bs > 8) return -1;
    const int64_t tr = (kBjBlock / bs) * bs;
    const int64_t nb = (n + bs - 1) / bs;
    for (int64_t i = 0; i < nb * bs; ++i) {               // row i = block i / bs, row i % bs of it
        const int64_t T = i / tr, t = i % tr;
        for (int j = 0; j < bs; ++j) {
            const int64_t cols = n - (i - i % bs);        // columns the block really has
            double v = (i % bs == j) ? 1.0 : 0.0;         // the identity around a short last block
            if (i < n && j < cols) v = laid[(T * bs + j) * kBjBlock + t];
            inv_blocks[i * bs + j] = v;
        }
    }
    return nb * bs * bs;
}

int launch_block_jacobi_build(hipStream_t st, double* blocks, int64_t n, int bs, const int* indptr, const int* col, const double* val,
                              long long* first_bad) {
    if (n <= 0) return 0;
    switch (bs) {
    case 1: launch_build<1>(st, blocks, n, indptr, col, val, first_bad); break;
    case 2: launch_build<2>(st, blocks, n, indptr, col, val, first_bad); break;
    case 3: launch_build<3>(st, blocks, n, indptr, col, val, first_bad); break;
    case 4: launch_build<4>(st, blocks, n, indptr, col, val, first_bad); break;
    case 5: launch_build<5>(st, blocks, n, indptr, col, val, first_bad); break;
    case 6: launch_build<6>(st, blocks, n, indptr, col, val, first_bad); break;
    case 7: launch_build<7>(st, blocks, n, indptr, col, val, first_bad); break;
    case 8: launch_build<8>(st, blocks, n, indptr, col, val, first_bad); break;
    default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_block_jacobi(hipStream_t st, double* dst, int dstride, const double* src, int sstride, int64_t n, int bs, const double* blocks) {
    if (n <= 0) return 0;
    switch (bs) {
    case 1: launch_one<1>(st, dst, dstride, src, sstride, n, blocks); break;
    case 2: launch_one<2>(st, dst, dstride, src, sstride, n, blocks); break;
    case 3: launch_one<3>(st, dst, dstride, src, sstride, n, blocks); break;
    case 4: launch_one<4>(st, dst, dstride, src, sstride, n, blocks); break;
    case 5: launch_one<5>(st, dst, dstride, src, sstride, n, blocks); break;
    case 6: launch_one<6>(st, dst, dstride, src, sstride, n, blocks); break;
    case 7: launch_one<7>(st, dst, dstride, src, sstride, n, blocks); break;
    case 8: launch_one<8>(st, dst, dstride, src, sstride, n, blocks); break;
    default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_block_jacobi_pair(hipStream_t st, double* wt, double* ut, const double* wu, int64_t n, int bs, const double* blocks, int mask,
                             const StopAt& stop) {
    if (n <= 0) return 0;
    switch (bs) {
    case 1: launch_two<1>(st, wt, ut, wu, n, blocks, mask, stop); break;
    case 2: launch_two<2>(st, wt, ut, wu, n, blocks, mask, stop); break;
    case 3: launch_two<3>(st, wt, ut, wu, n, blocks, mask, stop); break;
    case 4: launch_two<4>(st, wt, ut, wu, n, blocks, mask, stop); break;
    case 5: launch_two<5>(st, wt, ut, wu, n, blocks, mask, stop); break;
    case 6: launch_two<6>(st, wt, ut, wu, n, blocks, mask, stop); break;
    case 7: launch_two<7>(st, wt, ut, wu, n, blocks, mask, stop); break;
    case 8: launch_two<8>(st, wt, ut, wu, n, blocks, mask, stop); break;
    default: return -1;
    }
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace prcg
