// gfx950 (MI355X / CDNA4) kernels of the predict-and-recompute CG hot path.
//
// Everything here is HBM-bandwidth-bound fp64 streaming work (0.17-0.25 flop/byte):
// no MFMA.  What matters is 16-byte coalesced loads of val/col_ind, enough bytes in
// flight per CU, LDS-staged per-wavefront row reductions and wave64 shuffle reductions.
//
// Arithmetic contract (built with -ffp-contract=off): every update is `a + c*b` with
// the product rounded first and every SpMV row is summed left to right without FMA,
// exactly as NumPy / scipy._sparsetools.csr_matvec do in the reference
// (numerical_experiments/cg_variants/pipe_pr_cg.py:61-75, hs_cg.py:54-61), so vectors
// agree bit for bit with the reference given the same scalars; inner products use a
// fixed reduction tree (thread-sequential -> wave xor-butterfly -> waves in order ->
// blocks in order), deterministic run to run.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cstdlib>

#include "prcg_kernels.h"
#include "prcg_device.hpp"

namespace prcg {
namespace {

// ======================================================================================
// CSR-adaptive SpMV / two-vector SpMM.
// One wavefront per tile, persistent grid: wave `slot` handles tiles slot, slot+W, ...
// so the chip sweeps the matrix as one front (stencil neighbours are fetched while
// their lines are still in L2 / Infinity Cache).
//   stream phase : 16-B loads of 4 column indices and 4 values per lane, gather of
//                  x[col] (NV=2: one 16-B gather of the interleaved pair), products
//                  into this wave's LDS slice;
//   reduce phase : lane i sums row i of the tile sequentially from LDS and stores it.
// A row longer than a tile is summed by the whole wave (partial sums + butterfly).
// ======================================================================================
#ifndef PRCG_ROWSUM_UNROLL
#define PRCG_ROWSUM_UNROLL 8
#endif

template <int NV>
__device__ __forceinline__ typename VecT<NV>::type lds_row_sum(const typename VecT<NV>::type* my, int s, int e) {
    using V = typename VecT<NV>::type;
    V sum; vzero(sum);
    int q = s;
#if PRCG_ROWSUM_UNROLL >= 16
    for (; q + 16 <= e; q += 16) {
        V p[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) p[i] = my[q + i];
#pragma unroll
        for (int i = 0; i < 16; ++i) vacc(sum, p[i]);
    }
#endif
#if PRCG_ROWSUM_UNROLL >= 8
    for (; q + 8 <= e; q += 8) {   // 8 LDS reads in flight (medium rows: the read latency, not the adds, is the chain)
        const V p0 = my[q], p1 = my[q + 1], p2 = my[q + 2], p3 = my[q + 3];
        const V p4 = my[q + 4], p5 = my[q + 5], p6 = my[q + 6], p7 = my[q + 7];
        vacc(sum, p0); vacc(sum, p1); vacc(sum, p2); vacc(sum, p3);
        vacc(sum, p4); vacc(sum, p5); vacc(sum, p6); vacc(sum, p7);
    }
#endif
    for (; q + 4 <= e; q += 4) {   // 4 LDS reads in flight, adds stay in row order
        const V p0 = my[q], p1 = my[q + 1], p2 = my[q + 2], p3 = my[q + 3];
        vacc(sum, p0); vacc(sum, p1); vacc(sum, p2); vacc(sum, p3);
    }
    for (; q < e; ++q) vacc(sum, my[q]);
    return sum;
}

// ---- register image of one tile's val/col stream ------------------------------------
// Each lane holds 4 CONSECUTIVE nonzeros per step.  The image keeps the words AS LOADED
// (column words of the encoding in use, values or dictionary indices); they are decoded only
// when the tile is processed, one loop phase after the loads were issued -- a decode next to
// the load would make the compiler wait for the load right there and serialise the pipeline.
template <int C16> struct ColWord;
template <> struct ColWord<0> { int4 w; };          // the int32 indices given
template <> struct ColWord<16> { uint2 w; };        // 4 x 16-bit offsets from the tile's smallest column
template <> struct ColWord<8> { unsigned w; };      // 4 x 8-bit offsets

__device__ __forceinline__ int4 decode_cols(const ColWord<0>& c, int) { return c.w; }
// (entries of the chunk that belong to a neighbouring tile were encoded against ANOTHER base;
//  decoded against this one they still land inside the vector's kGatherPad spare entries, and
//  their products are never read)
__device__ __forceinline__ int4 decode_cols(const ColWord<16>& c, int b) {
    return make_int4(b + (int)(c.w.x & 0xffffu), b + (int)(c.w.x >> 16), b + (int)(c.w.y & 0xffffu), b + (int)(c.w.y >> 16));
}
__device__ __forceinline__ int4 decode_cols(const ColWord<8>& c, int b) {
    return make_int4(b + (int)(c.w & 255u), b + (int)((c.w >> 8) & 255u), b + (int)((c.w >> 16) & 255u), b + (int)(c.w >> 24));
}

// VD = true: the values arrive as 1-byte dictionary indices (4 per lane and step, one 32-bit
// load) plus ONE dictionary entry per lane and tile
template <int STEPS, int C16, bool VD>
struct MatRegs {
    ColWord<C16> c[STEPS];
    double2 va[STEPS], vb[STEPS];
};
template <int STEPS, int C16>
struct MatRegs<STEPS, C16, true> {
    ColWord<C16> c[STEPS];
    unsigned vi[STEPS];
    double dv;
};

// Tile descriptor: RawDesc = the words as loaded (two tiles ahead), TileDesc = the same made
// wave-uniform -- again one loop phase later, so that nobody waits for the load where it is issued.
struct RawDesc { int4 d; int base; int2 v; };
struct TileDesc { int rb, re, lo, hi, base, vo, vc; };

// (the three tables are separate __restrict__ const kernel arguments: wave-uniform loads from
//  them become scalar loads, which retire on their own counter instead of queueing behind the
//  vector loads and stores of the tile before)
template <int C16, bool VD>
__device__ __forceinline__ RawDesc read_raw(const int4* __restrict__ T4, const int* __restrict__ tbase,
                                            const int2* __restrict__ vdp, int t) {
    RawDesc r;
    r.d = T4[t];
    r.base = 0; r.v = make_int2(0, 0);
    if constexpr (C16 != 0) r.base = tbase[t];
    if constexpr (VD) r.v = vdp[t];
    return r;
}
__device__ __forceinline__ TileDesc cook(const RawDesc& r) {
    TileDesc o;
    o.rb = __builtin_amdgcn_readfirstlane(r.d.x); o.re = __builtin_amdgcn_readfirstlane(r.d.y);
    o.lo = __builtin_amdgcn_readfirstlane(r.d.z); o.hi = __builtin_amdgcn_readfirstlane(r.d.w);
    o.base = __builtin_amdgcn_readfirstlane(r.base);
    o.vo = __builtin_amdgcn_readfirstlane(r.v.x); o.vc = __builtin_amdgcn_readfirstlane(r.v.y);
    return o;
}

// Branch-free 16-byte (4-byte, 8-byte) loads of the tile's column words and values: a lane
// whose chunk lies past the tile re-reads the tile's first chunk (one hot line); its products
// land in LDS slots nobody reads.
// C16: width of the streamed column encoding: 0 = the int32 given, 16 / 8 = tile-relative offsets
template <int STEPS, int C16, bool VD>
__device__ __forceinline__ void load_tile_stream(const CsrDev& A, const TileDesc& d, int lane, MatRegs<STEPS, C16, VD>& m) {
    const int alo = d.lo & ~3;
    if constexpr (VD) m.dv = lane < d.vc ? A.vdict[d.vo + lane] : 0.0;
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
        const int base = alo + st * 256 + lane * 4;
        const int lb = base < d.hi ? base : alo;
        if constexpr (C16 == 8) m.c[st].w = *reinterpret_cast<const unsigned*>(A.col8 + lb);
        else if constexpr (C16 == 16) m.c[st].w = *reinterpret_cast<const uint2*>(A.col16 + lb);
        else m.c[st].w = *reinterpret_cast<const int4*>(A.col + lb);
        if constexpr (VD) {
            // 4 dictionary indices in 4 bytes (bytes of a neighbouring tile index ITS dictionary;
            // the lookup masks them into range and those products are never read)
            m.vi[st] = *reinterpret_cast<const unsigned*>(A.vidx8 + lb);
        } else {
            m.va[st] = *reinterpret_cast<const double2*>(A.val + lb);
            m.vb[st] = *reinterpret_cast<const double2*>(A.val + lb + 2);
        }
    }
}

// One tile: gather x[col], products -> this wave's LDS slice, then one lane per row sums
// its row left to right.  `cur` holds the tile's val/col stream (loaded one tile ago).
template <int NV, int EPI, int STEPS, int C16, bool VD>
__device__ __forceinline__ void process_tile(
    const CsrDev& A, const TileDesc& d, int lane, const MatRegs<STEPS, C16, VD>& cur,
    typename VecT<NV>::type* my, double* dict, const typename VecT<NV>::type* __restrict__ X,
    void* __restrict__ yout_, int write_mask, const double* __restrict__ ep_r,
    const double* __restrict__ ep_d, double* __restrict__ ep_st, double (&acc)[5], const Coefs& cf,
    const FusedRowPtrs& fr)
{
    using V = typename VecT<NV>::type;
    constexpr int kCap = 256 * STEPS - 3;
    const int rb = d.rb, re = d.re, lo = d.lo, hi = d.hi;
    if (hi - lo > kCap) {
        // ---- long row: the planner gives it a tile of its own (re == rb+1) ----------
        V sum; vzero(sum);
        for (int q = lo + lane; q < hi; q += 64) vacc(sum, vmul(A.val[q], X[A.col[q]]));
        sum = vwave_sum(sum);
        if (lane == 0) finish_row<NV, EPI>(rb, sum, yout_, write_mask, X, ep_r, ep_d, ep_st, acc, cf, fr);
        return;
    }
    const int alo = lo & ~3;   // 16-B aligned start; head slots < lo are never read
    // row pointers of the first two row batches (branch-free, clamped: issued now, waited
    // for only in the reduce phase)
    const int row0 = rb + lane, row1 = rb + 64 + lane;
    const int* ip0 = A.indptr + (row0 < re ? row0 : rb);
    const int* ip1 = A.indptr + (row1 < re ? row1 : rb);
    const int s0r = ip0[0], e0r = ip0[1], s1r = ip1[0], e1r = ip1[1];
    if constexpr (VD) {
        // the tile's dictionary: one entry per lane into this wave's LDS slot
        dict[lane] = cur.dv;
        wave_lds_sync();
    }
#pragma unroll
    for (int st = 0; st < STEPS; ++st) {
        const int4 cc = decode_cols(cur.c[st], d.base);
        const V g0 = X[cc.x], g1 = X[cc.y], g2 = X[cc.z], g3 = X[cc.w];
        double a0, a1, a2, a3;
        if constexpr (VD) {
            const unsigned v = cur.vi[st];
            a0 = dict[v & 63u]; a1 = dict[(v >> 8) & 63u]; a2 = dict[(v >> 16) & 63u]; a3 = dict[(v >> 24) & 63u];   // & 63: in range whatever the byte
        } else {
            a0 = cur.va[st].x; a1 = cur.va[st].y; a2 = cur.vb[st].x; a3 = cur.vb[st].y;
        }
        const int o = st * 256 + lane * 4;
        my[o + 0] = vmul(a0, g0);
        my[o + 1] = vmul(a1, g1);
        my[o + 2] = vmul(a2, g2);
        my[o + 3] = vmul(a3, g3);
    }
    wave_lds_sync();
    if (row0 < re) finish_row<NV, EPI>(row0, lds_row_sum<NV>(my, s0r - alo, e0r - alo), yout_, write_mask, X, ep_r, ep_d, ep_st, acc, cf, fr);
    if (row1 < re) finish_row<NV, EPI>(row1, lds_row_sum<NV>(my, s1r - alo, e1r - alo), yout_, write_mask, X, ep_r, ep_d, ep_st, acc, cf, fr);
    for (int row = rb + 128 + lane; row < re; row += 64) {
        const int s = A.indptr[row] - alo;
        const int e = A.indptr[row + 1] - alo;
        finish_row<NV, EPI>(row, lds_row_sum<NV>(my, s, e), yout_, write_mask, X, ep_r, ep_d, ep_st, acc, cf, fr);
    }
    wave_lds_sync();
}

// Software pipeline, two tiles deep: while a wave gathers / reduces tile t, the val/col
// stream of tile t+W is already in flight (second register image) and the descriptor of
// tile t+2W is being fetched.  The dependent chain per tile is then just
// gather -> LDS -> row sums, and every wave keeps HBM loads outstanding all the time.
// Everything loaded ahead stays RAW until the phase that needs it (see MatRegs / RawDesc).
template <int NV, int EPI, int STEPS, int C16, bool VD>
__global__ __launch_bounds__(kBlock) void k_spmv_tiles(
    CsrDev A, const Tile* __restrict__ tiles, const int* __restrict__ tbase, const int2* __restrict__ vdp, int ntiles,
    const void* __restrict__ xin_, void* __restrict__ yout_, int write_mask,
    const double* __restrict__ ep_r, const double* __restrict__ ep_d,
    double* __restrict__ ep_st, double* __restrict__ partials, double* __restrict__ aux,
    FusedPrev fz)
{
    using V = typename VecT<NV>::type;
    constexpr int kSlots = 256 * STEPS;
    constexpr int kCap = kSlots - 3;
    __shared__ V prod[kWaves][kSlots];
    __shared__ double dict_lds[VD ? kWaves : 1][VD ? kDictMax : 1];

    const V* __restrict__ X = reinterpret_cast<const V*>(xin_);
    const int4* __restrict__ T4 = reinterpret_cast<const int4*>(tiles);
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    V* my = prod[wv];
    double* dict = dict_lds[VD ? wv : 0];

    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    Coefs cf = {0.0, 0.0, 0.0};
    const FusedRowPtrs fr{reinterpret_cast<double2*>(yout_), reinterpret_cast<double2*>(ep_st), reinterpret_cast<double2*>(fz.rs),
                          ep_d, fz.w, fz.wt, (write_mask & 8) != 0};
    if constexpr (epi_product_stop(EPI)) { if (product_stopped<NV>(fz)) return; }      // (nothing loaded, nothing stored, no barrier met)
    if constexpr (epi_fused(EPI)) {
        // ep_r = the reduced inner products of the previous iteration; bit 2 of write_mask =
        // Meurant's prediction; aux = where alpha, beta, nu_pred of this iteration are kept
        // If the previous launch left one row of partial inner products per block, every block of THIS launch sums them
        // itself, in the same fixed order (thread t: rows t, t+256, ...; butterfly; waves in order: sum_prev_partials with four
        // waves IS that tree), so no separate reduction launch is needed and all blocks get bit-identical coefficients.  The
        // kernel boundary makes the partials visible; nothing is exchanged inside a launch.  A session with a stop word may end
        // here, before anything is loaded or stored (fused_prologue).
        if (!fused_prologue<kWaves>(fz, ep_r, (write_mask >> 2) & 1, aux, cf)) return;
    }

    // Tile order: wave `slot` takes tiles slot, slot+W, ... so the whole chip sweeps the
    // matrix as one front (stencil neighbours are fetched while their lines are still in
    // L2 / Infinity Cache).
    const int nblk = gridDim.x;
    const int W = nblk * kWaves;
    const int slot = xcd_remap(blockIdx.x, nblk) * kWaves + wv;
    const int tend = ntiles, step = W;
    int t = slot;

    MatRegs<STEPS, C16, VD> m0, m1;
    TileDesc d0 = {0, 0, 0, 0, 0, 0, 0}, d1 = {0, 0, 0, 0, 0, 0, 0};
    RawDesc rn = {make_int4(0, 0, 0, 0), 0, make_int2(0, 0)};     // raw descriptor of the tile after the current one
    if (t < tend) {
        d0 = cook(read_raw<C16, VD>(T4, tbase, vdp, t));
        if (d0.hi - d0.lo <= kCap) load_tile_stream<STEPS, C16, VD>(A, d0, lane, m0);
        if (t + step < tend) rn = read_raw<C16, VD>(T4, tbase, vdp, t + step);
    }

    while (t < tend) {
        // ---- even phase: tile t lives in m0 / d0; rn = raw descriptor of tile t+step (loaded a phase ago) ----
        {
            if (t + step < tend) {
                d1 = cook(rn);
                if (d1.hi - d1.lo <= kCap) load_tile_stream<STEPS, C16, VD>(A, d1, lane, m1);
            }
            const int t2 = t + 2 * step;
            rn = read_raw<C16, VD>(T4, tbase, vdp, t2 < tend ? t2 : t);
            process_tile<NV, EPI, STEPS, C16, VD>(A, d0, lane, m0, my, dict, X, yout_, write_mask, ep_r, ep_d, ep_st, acc, cf, fr);
            t += step;
        }
        if (t >= tend) break;
        // ---- odd phase: tile t lives in m1 / d1 ----
        {
            if (t + step < tend) {
                d0 = cook(rn);
                if (d0.hi - d0.lo <= kCap) load_tile_stream<STEPS, C16, VD>(A, d0, lane, m0);
            }
            const int t2 = t + 2 * step;
            rn = read_raw<C16, VD>(T4, tbase, vdp, t2 < tend ? t2 : t);
            process_tile<NV, EPI, STEPS, C16, VD>(A, d1, lane, m1, my, dict, X, yout_, write_mask, ep_r, ep_d, ep_st, acc, cf, fr);
            t += step;
        }
    }

    if constexpr (epi_fused(EPI)) { if constexpr (!epi_prec(EPI)) acc[4] = acc[3]; block_reduce_store<5>(acc, partials, 0); }
    else if constexpr (EPI == kEpiCG) block_reduce_store<5>(acc, partials, 0);
    else if constexpr (!epi_plain(EPI)) {
        double a3[3] = {acc[0], acc[1], acc[2]};
        block_reduce_store<3>(a3, partials, 0);
    }
}

// ======================================================================================
// Fused vector updates + inner products.  Block b owns `trips` consecutive 512-element
// trips; thread t handles elements 2t, 2t+1 of each trip with 16-byte accesses.
// ======================================================================================
// All state of the pipelined variants is stored as 16-byte pairs -- XP = (x,p), RS = (r,s),
// WU = (w,u), RSt = (r~,s~) -- so that every global access of this kernel is one fully
// coalesced 16-byte-per-lane instruction.  Thread t of block b handles elements
// base + t and base + 256 + t of each 512-element trip (two independent elements in
// flight).
template <bool PREC, bool DOTS_ONLY>
__global__ __launch_bounds__(kBlock) void k_pipe_update(PipeUpdateArgs a, int trips) {
    Coefs c = {0.0, 0.0, 0.0};
    if constexpr (!DOTS_ONLY) {
        c = predict(a.dots_prev, a.meurant);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            a.coef_out[0] = c.al; a.coef_out[1] = c.bt; a.coef_out[2] = c.nup;
        }
    }
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // mu, dl, gm, nu, rr
    const int64_t n = a.n;
    double2* __restrict__ XP = reinterpret_cast<double2*>(a.xp);
    double2* __restrict__ RS = reinterpret_cast<double2*>(a.rs);
    double2* __restrict__ RST = reinterpret_cast<double2*>(a.rst);
    double2* __restrict__ WU = reinterpret_cast<double2*>(a.wu);
    double* __restrict__ WT = a.wt;
    const double* __restrict__ D = a.d;
    const bool recompute_w = a.recompute_w != 0;

    int64_t base = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x;
    for (int j = 0; j < trips; ++j, base += kElemsPerTrip) {
        if (base >= n) break;
        // ---- loads of both elements first ----
        double2 xp[2], rs[2], wu[2], rst[2];
        double dv[2], wt[2], utv[2];
        bool ok[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t ie = base + e * kBlock;
            ok[e] = ie < n;
            const int64_t il = ok[e] ? ie : base;      // clamped: branch-free loads
            xp[e] = XP[il];
            rs[e] = RS[il];
            if constexpr (!DOTS_ONLY) wu[e] = WU[il];
            if constexpr (PREC) {
                rst[e] = RST[il];
                if constexpr (!DOTS_ONLY) {
                    if (a.ut) {              // preconditioner applied elsewhere (host callback): u~ and w~ are vectors
                        dv[e] = 0.0; utv[e] = a.ut[il]; wt[e] = WT[il];
                    } else {
                        dv[e] = D[il];
                        utv[e] = 0.0;
                        wt[e] = recompute_w ? 0.0 : WT[il];
                    }
                }
            }
        }
        // ---- arithmetic + stores, element 0 then element 1 (this order is part of the
        //      reduction tree the tests emulate) ----
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (!ok[e]) continue;
            const int64_t ie = base + e * kBlock;
            if constexpr (DOTS_ONLY) {
                if constexpr (PREC) {
                    acc[0] += xp[e].y * rs[e].y; acc[1] += rs[e].x * rst[e].y; acc[2] += rst[e].y * rs[e].y;
                    acc[3] += rst[e].x * rs[e].x; acc[4] += rs[e].x * rs[e].x;
                } else {
                    acc[0] += xp[e].y * rs[e].y; acc[1] += rs[e].x * rs[e].y; acc[2] += rs[e].y * rs[e].y;
                    acc[3] += rs[e].x * rs[e].x;
                }
            } else {
                const double xn = xp[e].x + c.al * xp[e].y;             // x += a p
                const double rn = rs[e].x - c.al * rs[e].y;             // r -= a s
                const double wn = wu[e].x - c.al * wu[e].y;             // w -= a u
                if constexpr (PREC) {
                    const double ut = a.ut ? utv[e] : dv[e] * wu[e].y;  // u~ = M^-1 u
                    const double wtv = a.ut ? wt[e] : (recompute_w ? dv[e] * wu[e].x : wt[e]);   // w~
                    const double rtn = rst[e].x - c.al * rst[e].y;      // r~ -= a s~
                    const double wtn = wtv - c.al * ut;                 // w~ -= a u~
                    const double pn = rtn + c.bt * xp[e].y;             // p = r~ + b p
                    const double sn = wn + c.bt * rs[e].y;              // s = w + b s
                    const double stn = wtn + c.bt * rst[e].y;           // s~ = w~ + b s~
                    XP[ie] = make_double2(xn, pn);
                    RS[ie] = make_double2(rn, sn);
                    RST[ie] = make_double2(rtn, stn);
                    if (!recompute_w) { a.wu[2 * ie] = wn; WT[ie] = wtn; }
                    acc[0] += pn * sn; acc[1] += rn * stn; acc[2] += stn * sn;
                    acc[3] += rtn * rn; acc[4] += rn * rn;
                } else {
                    const double pn = rn + c.bt * xp[e].y;              // p = r + b p
                    const double sn = wn + c.bt * rs[e].y;              // s = w + b s
                    XP[ie] = make_double2(xn, pn);
                    RS[ie] = make_double2(rn, sn);
                    if (!recompute_w) a.wu[2 * ie] = wn;
                    acc[0] += pn * sn; acc[1] += rn * sn; acc[2] += sn * sn; acc[3] += rn * rn;
                }
            }
        }
    }
    if constexpr (!PREC) acc[4] = acc[3];
    block_reduce_store<5>(acc, a.partials, 0);
}

// The stop form of the STORED-TILDE flavour (launch_pipe_update with a stop, prcg_kernels.h): update k of a block-Jacobi session begun with
// a threshold (prcg_set_stop_block_jacobi).  A kernel of its own: k_pipe_update above stays as it is, instruction for instruction.
// The word is tested first: the reduction that closed an earlier iteration wrote it (k_reduce_final_stop), so it was complete before
// this launch began, every wave reads the same value through readfirstlane, and a workgroup leaves as a whole on a scalar branch --
// before anything is loaded or stored and before the one barrier (block_reduce_store).  Behind the head: k_pipe_update<true, false>
// with a.ut set and a.d null -- u~ and w~ loaded as vectors -- the same expressions in the same order (multiply, then add), the same
// element order, the same accumulators and the same tree: the bits of that kernel in every vector and every partial row.
__global__ __launch_bounds__(kBlock) void k_pipe_update_stop(PipeUpdateArgs a, int trips, const int* __restrict__ word, int k) {
    const int at = __builtin_amdgcn_readfirstlane(word[0]);
    if (at >= 0 && at < k) return;
    const Coefs c = predict(a.dots_prev, a.meurant);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.coef_out[0] = c.al; a.coef_out[1] = c.bt; a.coef_out[2] = c.nup;
    }
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // mu, dl, gm, nu, rr
    const int64_t n = a.n;
    double2* __restrict__ XP = reinterpret_cast<double2*>(a.xp);
    double2* __restrict__ RS = reinterpret_cast<double2*>(a.rs);
    double2* __restrict__ RST = reinterpret_cast<double2*>(a.rst);
    double2* __restrict__ WU = reinterpret_cast<double2*>(a.wu);
    double* __restrict__ WT = a.wt;
    const double* __restrict__ UT = a.ut;
    const bool recompute_w = a.recompute_w != 0;

    int64_t base = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x;
    for (int j = 0; j < trips; ++j, base += kElemsPerTrip) {
        if (base >= n) break;
        double2 xp[2], rs[2], wu[2], rst[2];
        double wt[2], ut[2];
        bool ok[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t ie = base + e * kBlock;
            ok[e] = ie < n;
            const int64_t il = ok[e] ? ie : base;      // clamped: branch-free loads
            xp[e] = XP[il]; rs[e] = RS[il]; wu[e] = WU[il]; rst[e] = RST[il];
            ut[e] = UT[il]; wt[e] = WT[il];
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {                  // element 0 then element 1: part of the reduction tree
            if (!ok[e]) continue;
            const int64_t ie = base + e * kBlock;
            const double xn = xp[e].x + c.al * xp[e].y;             // x += a p
            const double rn = rs[e].x - c.al * rs[e].y;             // r -= a s
            const double wn = wu[e].x - c.al * wu[e].y;             // w -= a u
            const double rtn = rst[e].x - c.al * rst[e].y;          // r~ -= a s~
            const double wtn = wt[e] - c.al * ut[e];                // w~ -= a u~
            const double pn = rtn + c.bt * xp[e].y;                 // p = r~ + b p
            const double sn = wn + c.bt * rs[e].y;                  // s = w + b s
            const double stn = wtn + c.bt * rst[e].y;               // s~ = w~ + b s~
            XP[ie] = make_double2(xn, pn);
            RS[ie] = make_double2(rn, sn);
            RST[ie] = make_double2(rtn, stn);
            if (!recompute_w) { a.wu[2 * ie] = wn; WT[ie] = wtn; }
            acc[0] += pn * sn; acc[1] += rn * stn; acc[2] += stn * sn;
            acc[3] += rtn * rn; acc[4] += rn * rn;
        }
    }
    block_reduce_store<5>(acc, a.partials, 0);
}

// ---- Hestenes-Stiefel (hs_cg.py:54-61, hs_pcg :116-124) ------------------------------
template <bool PREC, bool DOTS_ONLY>
__global__ __launch_bounds__(kBlock) void k_hs_update_xr(HsArgs a, int trips, const double* __restrict__ prev_mu, int nprev,
                                                         double* dots_prev_w) {
    double al = 0.0;
    if constexpr (!DOTS_ONLY) {
        double mu;
        if (nprev > 0) {
            // mu = <p,s> of the previous iteration: still the product launch's block partials
            double m[1];
            sum_prev_partials<1, kWaves>(prev_mu, nprev, 0, m);
            mu = m[0];
            if (blockIdx.x == 0 && threadIdx.x == 0) dots_prev_w[0] = mu;
        } else {
            mu = a.dots_prev[0];
        }
        al = a.dots_prev[3] / mu;                               // a_k1 = nu/mu
        if (blockIdx.x == 0 && threadIdx.x == 0) a.coef_out[0] = al;
    }
    double acc[2] = {0.0, 0.0};   // nu, rr
    int64_t i = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x * 2;
    for (int j = 0; j < trips; ++j, i += kElemsPerTrip) {
        if (i + 1 < a.n) {
            // the thread's two elements as 16-byte loads and stores (same expressions, same order of the sums: element i, then i + 1)
            double2 rn = *reinterpret_cast<const double2*>(a.r + i);
            if constexpr (!DOTS_ONLY) {
                const double2 x2 = *reinterpret_cast<const double2*>(a.x + i), p2 = *reinterpret_cast<const double2*>(a.p + i);
                const double2 s2 = *reinterpret_cast<const double2*>(a.s + i);
                *reinterpret_cast<double2*>(a.x + i) = make_double2(x2.x + al * p2.x, x2.y + al * p2.y);
                rn = make_double2(rn.x - al * s2.x, rn.y - al * s2.y);
                *reinterpret_cast<double2*>(a.r + i) = rn;
            }
            if constexpr (PREC) {
                const double2 d2 = *reinterpret_cast<const double2*>(a.d + i);
                const double2 z = make_double2(d2.x * rn.x, d2.y * rn.y);      // r~ = M^-1 r
                *reinterpret_cast<double2*>(a.rt + i) = z;
                acc[0] += rn.x * z.x; acc[1] += rn.x * rn.x;
                acc[0] += rn.y * z.y; acc[1] += rn.y * rn.y;
            } else {
                acc[0] += rn.x * rn.x;
                acc[0] += rn.y * rn.y;
            }
        } else if (i < a.n) {
            double rn = a.r[i];
            if constexpr (!DOTS_ONLY) {
                a.x[i] = a.x[i] + al * a.p[i];
                rn = rn - al * a.s[i];
                a.r[i] = rn;
            }
            if constexpr (PREC) {
                const double z = a.d[i] * rn;
                a.rt[i] = z;
                acc[0] += rn * z; acc[1] += rn * rn;
            } else {
                acc[0] += rn * rn;
            }
        }
    }
    if constexpr (!PREC) acc[1] = acc[0];
    block_reduce_store<2>(acc, a.partials, 3);
}

__global__ __launch_bounds__(kBlock) void k_hs_update_p(HsArgs a, int trips, const double* __restrict__ prev_nu, int nprev,
                                                        double* dots_cur_w) {
    double nu;
    if (nprev > 0) {
        double m[2];
        sum_prev_partials<2, kWaves>(prev_nu, nprev, 3, m);     // nu_k, rr_k: still the update launch's block partials
        nu = m[0];
        if (blockIdx.x == 0 && threadIdx.x == 0) { dots_cur_w[3] = m[0]; dots_cur_w[4] = m[1]; }
    } else {
        nu = a.dots_cur[3];
    }
    const double bt = nu / a.dots_prev[3];                      // b_k = nu_k / nu_k1
    if (blockIdx.x == 0 && threadIdx.x == 0) a.coef_out[1] = bt;
    const double* __restrict__ z = a.rt ? a.rt : a.r;
    int64_t i = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x * 2;
    for (int j = 0; j < trips; ++j, i += kElemsPerTrip) {
        if (i + 1 < a.n) {                                      // the thread's two elements as 16-byte loads and stores
            const double2 z2 = *reinterpret_cast<const double2*>(z + i), p2 = *reinterpret_cast<const double2*>(a.p + i);
            *reinterpret_cast<double2*>(a.p + i) = make_double2(z2.x + bt * p2.x, z2.y + bt * p2.y);     // p = r~ + b p
        } else if (i < a.n) {
            a.p[i] = z[i] + bt * a.p[i];
        }
    }
}

// The stop forms (launch_hs_update_xr / launch_hs_update_p with a stop, prcg_kernels.h): iteration k of a Hestenes-Stiefel session begun with
// a threshold (prcg_set_stop_hs).  Kernels of their own: the two above stay as they are, instruction for instruction.  Behind their
// heads they are the statements of k_hs_update_xr<PREC, false> and k_hs_update_p in their order -- the same expressions, the same
// element order, the same accumulators and the same tree: the bits of those kernels in every vector and every partial row.
// k_hs_update_xr_stop is launch A of iteration k and closes iteration k - 1:
//  1. The word names an iteration BEFORE k - 1: the session stopped in an earlier launch.  The word was complete before this launch
//     began (kernel boundary), so every wave of every workgroup reads the same value and leaves here, before any barrier and before
//     anything is written.  (A word that names k - 1 itself was left by the reduction that ended the last prcg_iterate call or by the
//     session's start -- then mu is read reduced, the rule below fires again and nothing is written -- or it is the store of
//     workgroup 0 of THIS launch seen by a wave that started late: it goes on and reaches that verdict itself, with the rest of its
//     workgroup.  Leaving on it here would let waves of one workgroup part BEFORE the barriers of the sum: fused_prologue.)
//  2. The rule on row k - 1 = {mu, nu, rr}.  mu is the same bits in every thread of every workgroup (one tree over one buffer, read
//     behind the barrier that completes it; or one load of a reduced word), nu and rr are loads of words that workgroup 0 of the
//     launch before (or the session's start) stored before the kernel boundary, thr is a kernel argument: every wave of the launch
//     reaches the same verdict (readfirstlane: a scalar branch), behind the last barrier of the sum and before the next one, so
//     whole workgroups leave together.  Thread 0 of workgroup 0 records {k - 1, status}; mu of k - 1 has been stored (it belongs
//     to the state of the stop); a_k, x, r, r~ and the partial rows of iteration k are not touched.
// k_hs_update_p_stop decides nothing (mu_k does not exist before the product has run): it leaves at once, on a scalar branch and
// before its sum, if the session stopped before k.
template <bool PREC>
__global__ __launch_bounds__(kBlock) void k_hs_update_xr_stop(HsArgs a, int trips, const double* __restrict__ prev_mu, int nprev,
                                                              double* dots_prev_w, SmallStop stop, int k) {
    const int at = __builtin_amdgcn_readfirstlane(stop.word[0]);
    if (at >= 0 && at < k - 1) return;                          // 1.
    double mu;
    if (nprev > 0) {
        // mu = <p,s> of the previous iteration: still the product launch's block partials
        double m[1];
        sum_prev_partials<1, kWaves>(prev_mu, nprev, 0, m);
        mu = m[0];
        if (blockIdx.x == 0 && threadIdx.x == 0) dots_prev_w[0] = mu;
    } else {
        mu = a.dots_prev[0];
    }
    const int verdict = stop_rule(mu, a.dots_prev[3], a.dots_prev[4], stop.thr);      // 2.
    if (verdict) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { stop.word[0] = k - 1; stop.word[1] = verdict; }
        return;
    }
    const double al = a.dots_prev[3] / mu;                      // a_k1 = nu/mu
    if (blockIdx.x == 0 && threadIdx.x == 0) a.coef_out[0] = al;
    double acc[2] = {0.0, 0.0};   // nu, rr
    int64_t i = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x * 2;
    for (int j = 0; j < trips; ++j, i += kElemsPerTrip) {
        if (i + 1 < a.n) {
            // the thread's two elements as 16-byte loads and stores (same expressions, same order of the sums: element i, then i + 1)
            double2 rn = *reinterpret_cast<const double2*>(a.r + i);
            const double2 x2 = *reinterpret_cast<const double2*>(a.x + i), p2 = *reinterpret_cast<const double2*>(a.p + i);
            const double2 s2 = *reinterpret_cast<const double2*>(a.s + i);
            *reinterpret_cast<double2*>(a.x + i) = make_double2(x2.x + al * p2.x, x2.y + al * p2.y);
            rn = make_double2(rn.x - al * s2.x, rn.y - al * s2.y);
            *reinterpret_cast<double2*>(a.r + i) = rn;
            if constexpr (PREC) {
                const double2 d2 = *reinterpret_cast<const double2*>(a.d + i);
                const double2 z = make_double2(d2.x * rn.x, d2.y * rn.y);      // r~ = M^-1 r
                *reinterpret_cast<double2*>(a.rt + i) = z;
                acc[0] += rn.x * z.x; acc[1] += rn.x * rn.x;
                acc[0] += rn.y * z.y; acc[1] += rn.y * rn.y;
            } else {
                acc[0] += rn.x * rn.x;
                acc[0] += rn.y * rn.y;
            }
        } else if (i < a.n) {
            double rn = a.r[i];
            a.x[i] = a.x[i] + al * a.p[i];
            rn = rn - al * a.s[i];
            a.r[i] = rn;
            if constexpr (PREC) {
                const double z = a.d[i] * rn;
                a.rt[i] = z;
                acc[0] += rn * z; acc[1] += rn * rn;
            } else {
                acc[0] += rn * rn;
            }
        }
    }
    if constexpr (!PREC) acc[1] = acc[0];
    block_reduce_store<2>(acc, a.partials, 3);
}

__global__ __launch_bounds__(kBlock) void k_hs_update_p_stop(HsArgs a, int trips, const double* __restrict__ prev_nu, int nprev,
                                                             double* dots_cur_w, const int* __restrict__ word, int k) {
    const int at = __builtin_amdgcn_readfirstlane(word[0]);
    if (at >= 0 && at < k) return;
    double nu;
    if (nprev > 0) {
        double m[2];
        sum_prev_partials<2, kWaves>(prev_nu, nprev, 3, m);     // nu_k, rr_k: still the update launch's block partials
        nu = m[0];
        if (blockIdx.x == 0 && threadIdx.x == 0) { dots_cur_w[3] = m[0]; dots_cur_w[4] = m[1]; }
    } else {
        nu = a.dots_cur[3];
    }
    const double bt = nu / a.dots_prev[3];                      // b_k = nu_k / nu_k1
    if (blockIdx.x == 0 && threadIdx.x == 0) a.coef_out[1] = bt;
    const double* __restrict__ z = a.rt ? a.rt : a.r;
    int64_t i = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x * 2;
    for (int j = 0; j < trips; ++j, i += kElemsPerTrip) {
        if (i + 1 < a.n) {                                      // the thread's two elements as 16-byte loads and stores
            const double2 z2 = *reinterpret_cast<const double2*>(z + i), p2 = *reinterpret_cast<const double2*>(a.p + i);
            *reinterpret_cast<double2*>(a.p + i) = make_double2(z2.x + bt * p2.x, z2.y + bt * p2.y);     // p = r~ + b p
        } else if (i < a.n) {
            a.p[i] = z[i] + bt * a.p[i];
        }
    }
}

// ---- non-pipelined predict-and-recompute (pr_cg.py:146-151) ---------------------------
template <bool PREC, bool DOTS_ONLY>
__global__ __launch_bounds__(kBlock) void k_pr_update(PrArgs a, int trips) {
    Coefs c = {0.0, 0.0, 0.0};
    if constexpr (!DOTS_ONLY) {
        c = predict(a.dots_prev, a.meurant);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            a.coef_out[0] = c.al; a.coef_out[1] = c.bt; a.coef_out[2] = c.nup;
        }
    }
    double acc[2] = {0.0, 0.0};   // nu = r~.r, rr
    int64_t i = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x * 2;
    for (int j = 0; j < trips; ++j, i += kElemsPerTrip) {
        if (i + 1 < a.n) {
            // the thread's two elements as 16-byte loads and stores (same expressions, sums in the order element i, then i + 1)
            double2 rn = *reinterpret_cast<const double2*>(a.r + i);
            double2 rtn = rn;
            if constexpr (PREC) rtn = *reinterpret_cast<const double2*>(a.rt + i);
            if constexpr (!DOTS_ONLY) {
                const double2 x2 = *reinterpret_cast<const double2*>(a.x + i), p2 = *reinterpret_cast<const double2*>(a.p + i);
                const double2 s2 = *reinterpret_cast<const double2*>(a.s + i);
                *reinterpret_cast<double2*>(a.x + i) = make_double2(x2.x + c.al * p2.x, x2.y + c.al * p2.y);
                rn = make_double2(rn.x - c.al * s2.x, rn.y - c.al * s2.y);
                *reinterpret_cast<double2*>(a.r + i) = rn;
                if constexpr (PREC) {
                    const double2 st2 = *reinterpret_cast<const double2*>(a.st_ + i);
                    rtn = make_double2(rtn.x - c.al * st2.x, rtn.y - c.al * st2.y);
                    *reinterpret_cast<double2*>(a.rt + i) = rtn;
                } else {
                    rtn = rn;
                }
                *reinterpret_cast<double2*>(a.p + i) = make_double2(rtn.x + c.bt * p2.x, rtn.y + c.bt * p2.y);
            }
            acc[0] += rtn.x * rn.x; acc[1] += rn.x * rn.x;
            acc[0] += rtn.y * rn.y; acc[1] += rn.y * rn.y;
        } else if (i < a.n) {
            double rn = a.r[i];
            double rtn = PREC ? a.rt[i] : rn;
            if constexpr (!DOTS_ONLY) {
                a.x[i] = a.x[i] + c.al * a.p[i];
                rn = rn - c.al * a.s[i];
                a.r[i] = rn;
                if constexpr (PREC) {
                    rtn = rtn - c.al * a.st_[i];
                    a.rt[i] = rtn;
                } else {
                    rtn = rn;
                }
                a.p[i] = rtn + c.bt * a.p[i];
            }
            acc[0] += rtn * rn; acc[1] += rn * rn;
        }
    }
    block_reduce_store<2>(acc, a.partials, 3);
}

// ---- competitor baselines: Chronopoulos-Gear (cg_cg.py:59-68) and Ghysels-Vanroose
//      (gv_cg.py:65-81).  mu is a RECURRENCE here, not an inner product:
//      mu_k = eta_k - (b_k / a_k1) nu_k, computed by thread 0 and stored with the scalars. ----
__global__ __launch_bounds__(kBlock) void k_cg_update_ps(CgArgs a, int trips, const double* __restrict__ prev, int nprev) {
    // dots_prev: nu_k1 (slot 3), mu_k1 (slot 0); dots_cur: nu_k (3), eta_k (1)
    const double al = a.dots_prev[3] / a.dots_prev[0];          // a_k1
    double nu, eta;
    if (nprev > 0) {
        double m[5];
        sum_prev_partials<5, kWaves>(prev, nprev, 0, m);        // the product launch's block partials
        nu = m[3]; eta = m[1];
        if (blockIdx.x == 0 && threadIdx.x == 0) { a.dots_cur_w[1] = m[1]; a.dots_cur_w[3] = m[3]; a.dots_cur_w[4] = m[4]; }
    } else {
        nu = a.dots_cur[3]; eta = a.dots_cur[1];
    }
    const double bt = nu / a.dots_prev[3];                      // b_k
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.coef_out[0] = al; a.coef_out[1] = bt;
        a.dots_cur_w[0] = eta - (bt / al) * nu;                 // mu_k
    }
    const double* __restrict__ z = a.z;
    int64_t i = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x * 2;
    auto axpby2 = [bt](double* __restrict__ y, const double* __restrict__ x, int64_t at) {      // y = x + b y on two elements, 16 bytes each way
        const double2 x2 = *reinterpret_cast<const double2*>(x + at), y2 = *reinterpret_cast<const double2*>(y + at);
        *reinterpret_cast<double2*>(y + at) = make_double2(x2.x + bt * y2.x, x2.y + bt * y2.y);
    };
    for (int j = 0; j < trips; ++j, i += kElemsPerTrip) {
        if (i + 1 < a.n) {
            axpby2(a.p, z, i);                                  // p = r~ + b p
            axpby2(a.s, a.w, i);                                // s = w + b s
            if (a.st_) axpby2(a.st_, a.wt, i);                  // s~ = w~ + b s~   (gv_pcg)
            if (a.u) axpby2(a.u, a.t, i);                       // u = t + b u      (gv)
        } else if (i < a.n) {
            a.p[i] = z[i] + bt * a.p[i];
            a.s[i] = a.w[i] + bt * a.s[i];
            if (a.st_) a.st_[i] = a.wt[i] + bt * a.st_[i];
            if (a.u) a.u[i] = a.t[i] + bt * a.u[i];
        }
    }
}

// gv: x += a p; r -= a s; r~ -= a s~; w -= a u; w~ = M^-1 w; partials nu = r.r~, eta = w.r~, r.r
template <bool PREC, bool DOTS_ONLY>
__global__ __launch_bounds__(kBlock) void k_gv_update1(CgArgs a, int trips) {
    double al = 0.0;
    if constexpr (!DOTS_ONLY) al = a.dots_prev[3] / a.dots_prev[0];
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};   // slots: -, eta, -, nu, rr
    int64_t i = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x * 2;
    for (int j = 0; j < trips; ++j, i += kElemsPerTrip) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t ie = i + e;
            if (ie >= a.n) break;
            double rn = a.r[ie], wn = a.w[ie];
            double zn = PREC ? a.rt[ie] : rn;
            if constexpr (!DOTS_ONLY) {
                a.x[ie] = a.x[ie] + al * a.p[ie];
                rn = rn - al * a.s[ie];
                a.r[ie] = rn;
                wn = wn - al * a.u[ie];
                a.w[ie] = wn;
                if constexpr (PREC) {
                    zn = zn - al * a.st_[ie];
                    a.rt[ie] = zn;
                    if (a.d) a.wt[ie] = a.d[ie] * wn;        // (null: w~ = M^-1 w is applied by the caller afterwards)
                } else {
                    zn = rn;
                }
            }
            // gv_pcg's initial eta is w.r, its loop's eta is w.r~ (gv_cg.py:107 vs :163)
            acc[1] += wn * ((DOTS_ONLY && PREC) ? rn : zn);
            acc[3] += rn * zn; acc[4] += rn * rn;
        }
    }
    block_reduce_store<5>(acc, a.partials, 0);
}

// ---- fixed-order final reduction of per-block partials --------------------------------
constexpr int kFinalThreads = 256;   // same tree as the fused last-block reduction
// the tree up to the four wave sums of every slot (red), complete behind the barrier; slot q's total is red[0][q] + red[1][q] +
// red[2][q] + red[3][q], added in that order by whoever needs it
// (the part of the tree behind a thread's own rows: butterfly per wave, the wave sums parked in red, the barrier -- shared by
// every walk over the rows, so that none of them can drift from the others)
__device__ __forceinline__ void reduce_final_wave_sums(const double (&acc)[kPartialStride], double (&red)[kFinalThreads / 64][kPartialStride])
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < kPartialStride; ++q) {
        const double v = wave_sum(acc[q]);
        if (lane == 0) red[wv][q] = v;
    }
    __syncthreads();
}
__device__ __forceinline__ void reduce_final_waves(const double* __restrict__ partials, int nparts, int src_first, int count,
                                                   double (&red)[kFinalThreads / 64][kPartialStride])
{
    double acc[kPartialStride];
#pragma unroll
    for (int q = 0; q < kPartialStride; ++q) acc[q] = 0.0;
    for (int j = threadIdx.x; j < nparts; j += kFinalThreads) {
#pragma unroll
        for (int q = 0; q < kPartialStride; ++q)
            if (q < count) acc[q] += partials[(size_t)j * kPartialStride + src_first + q];
    }
    reduce_final_wave_sums(acc, red);
}
__device__ __forceinline__ double reduce_final_total(const double (&red)[kFinalThreads / 64][kPartialStride], int q) {
    double v = red[0][q];
    for (int w = 1; w < kFinalThreads / 64; ++w) v += red[w][q];
    return v;
}
__global__ __launch_bounds__(kFinalThreads) void k_reduce_final(
    const double* __restrict__ partials, int nparts, double* __restrict__ out,
    int src_first, int dst_first, int count)
{
    __shared__ double red[kFinalThreads / 64][kPartialStride];
    reduce_final_waves(partials, nparts, src_first, count, red);
    if ((int)threadIdx.x < count) out[dst_first + threadIdx.x] = reduce_final_total(red, threadIdx.x);
}
// several independent reductions in one launch (launch_reduce_final_jobs): workgroup b is k_reduce_final with job b's arguments.
// The jobs of the block-Jacobi multi-RHS sessions have one partial row per TILE (16 090 at n = 4.1 M: 63 rows per thread), and a
// thread's rows are 256 rows apart, so the walk is a chain of load latencies.  Here a thread has the loads of kFinalBatch of its
// rows in flight before it adds them -- the same rows, added in the same order into the same accumulators as reduce_final_waves
// adds them (a row past the end is loaded from a clamped index and not added), then reduce_final_wave_sums and reduce_final_total,
// the very code k_reduce_final runs: hence the same bits.
constexpr int kFinalBatch = 8;
__global__ __launch_bounds__(kFinalThreads) void k_reduce_final_jobs(ReduceJobs jobs)
{
    __shared__ double red[kFinalThreads / 64][kPartialStride];
    ReduceJob j = jobs.job[0];
#pragma unroll
    for (int q = 1; q < kMaxReduceJobs; ++q)
        if ((int)blockIdx.x == q) j = jobs.job[q];
    const double* __restrict__ partials = j.partials;
    double acc[kPartialStride];
#pragma unroll
    for (int q = 0; q < kPartialStride; ++q) acc[q] = 0.0;
    for (int r0 = threadIdx.x; r0 < j.nparts; r0 += kFinalBatch * kFinalThreads) {
        double v[kFinalBatch][kPartialStride];
#pragma unroll
        for (int u = 0; u < kFinalBatch; ++u) {
            const int r = r0 + u * kFinalThreads;
            const size_t rl = r < j.nparts ? r : r0;
#pragma unroll
            for (int q = 0; q < kPartialStride; ++q) v[u][q] = q < j.count ? partials[rl * kPartialStride + j.src_first + q] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < kFinalBatch; ++u) {
            if (r0 + u * kFinalThreads < j.nparts) {
#pragma unroll
                for (int q = 0; q < kPartialStride; ++q)
                    if (q < j.count) acc[q] += v[u][q];
            }
        }
    }
    reduce_final_wave_sums(acc, red);
    if ((int)threadIdx.x < j.count) j.out[j.dst_first + threadIdx.x] = reduce_final_total(red, threadIdx.x);
}
// The stop form (launch_reduce_final with a stop, prcg_kernels.h): the five sums of a pipelined iteration by the code above, then the
// rule on them.  The word is tested first: it was complete before this launch began (only a launch's end or this kernel's thread 0
// writes it), so all four waves read the same value and leave together, before the barrier.  Thread 0 then adds the wave sums of
// mu, nu, rr in the order threads 0, 3, 4 add them: the bits they store, and the bits the next launch's prologue would have had.
__global__ __launch_bounds__(kFinalThreads) void k_reduce_final_stop(
    const double* __restrict__ partials, int nparts, double* __restrict__ out, SmallStop stop, int k)
{
    if (__builtin_amdgcn_readfirstlane(stop.word[0]) >= 0) return;
    __shared__ double red[kFinalThreads / 64][kPartialStride];
    reduce_final_waves(partials, nparts, 0, 5, red);
    if (threadIdx.x < 5) out[threadIdx.x] = reduce_final_total(red, threadIdx.x);
    if (threadIdx.x == 0) {
        const int verdict = stop_rule(reduce_final_total(red, 0), reduce_final_total(red, 3), reduce_final_total(red, 4), stop.thr);
        if (verdict) { stop.word[0] = k; stop.word[1] = verdict; }
    }
}

// The stop form of the ONE-slot reduction that closes a Hestenes-Stiefel iteration (launch_reduce_hs_mu with a stop, prcg_kernels.h): mu_k
// from the product launch's partials by the code of k_reduce_final -- the same tree, the same bits --, stored to row[0]; nu_k and
// rr_k are read from the row, where the launch before stored them (kernel boundary); then the rule.  The word is tested first, as in
// k_reduce_final_stop: all four waves read the same value and leave together, before the barrier.
__global__ __launch_bounds__(kFinalThreads) void k_reduce_hs_mu_stop(
    const double* __restrict__ partials, int nparts, double* __restrict__ row, SmallStop stop, int k)
{
    if (__builtin_amdgcn_readfirstlane(stop.word[0]) >= 0) return;
    __shared__ double red[kFinalThreads / 64][kPartialStride];
    reduce_final_waves(partials, nparts, 0, 1, red);
    if (threadIdx.x == 0) {
        const double mu = reduce_final_total(red, 0);
        row[0] = mu;
        const int verdict = stop_rule(mu, row[3], row[4], stop.thr);
        if (verdict) { stop.word[0] = k; stop.word[1] = verdict; }
    }
}

// ---- merged exchange (small halos) -----------------------------------------------------
// One all-gather per iteration carries both the rank's five partial inner products and the
// (r,s) rows its neighbours need.  Slot layout per rank: 8 doubles (sums 0..4, 3 pad), then
// the packed rows as pairs.
// pack: the fixed-order reduction of k_reduce_final, written into the slot header, plus the rows.
__global__ __launch_bounds__(kFinalThreads) void k_gather_pack(
    const double* __restrict__ partials, int nparts, double* __restrict__ slot,
    const double2* __restrict__ rs, const int* __restrict__ send_idx, int nsend)
{
    __shared__ double red[kFinalThreads / 64][kPartialStride];
    double acc[kPartialStride];
#pragma unroll
    for (int q = 0; q < kPartialStride; ++q) acc[q] = 0.0;
    for (int j = threadIdx.x; j < nparts; j += kFinalThreads) {
#pragma unroll
        for (int q = 0; q < kPartialStride; ++q)
            if (q < 5) acc[q] += partials[(size_t)j * kPartialStride + q];
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < kPartialStride; ++q) {
        const double v = wave_sum(acc[q]);
        if (lane == 0) red[wv][q] = v;
    }
    __syncthreads();
    if ((int)threadIdx.x < 5) {
        double v = red[0][threadIdx.x];
        for (int w = 1; w < kFinalThreads / 64; ++w) v += red[w][threadIdx.x];
        slot[threadIdx.x] = v;
    }
    double2* rows = reinterpret_cast<double2*>(slot + 8);
    for (int j = threadIdx.x; j < nsend; j += kFinalThreads) rows[j] = rs[send_idx[j]];
}

// unpack: global sums = the ranks' partial sums added in rank order (the same bits on every
// rank, whatever algorithm RCCL picked for the transport); ghost rows copied into place.
// Publication for waves that WAIT inside a running launch (cdna_hip_programming.md Guideline 16, the
// all-write-through form): payload and counter are stored with agent-scope atomic stores (sc1: they
// leave the XCD's L2), the storing wave drains them before the counter goes out, and the readers
// (k_win_tiles, deferred form) use agent-scope atomic loads for the counter AND the payload.
// The record is REPLICATED kPubCopies times, one copy per 64-byte line: thousands of waves poll, and they
// spread over the copies (one hot word would saturate its L2 channel and delay the very store they wait for).
__device__ __forceinline__ void publish(double* pub, double v, int nvals, unsigned value) {
    // called by ONE wave; lane q < nvals holds value q; lane c writes copy c
    const int lane = threadIdx.x & 63;
    double* mine = pub + (size_t)lane * 8;
#pragma unroll
    for (int q = 0; q < 5; ++q) {
        const double vq = __shfl(v, q, 64);
        if (q < nvals) __hip_atomic_store(mine + q, vq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // every lane's payload has left before its counter does
    __hip_atomic_store(reinterpret_cast<unsigned*>(mine + 6), value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kFinalThreads) void k_gather_unpack(
    const double* __restrict__ gbuf, int slot_doubles, int nranks, double* __restrict__ dots_out,
    double2* __restrict__ rs_ghost, const int* __restrict__ ghost_src, int nghost, double* pub, unsigned pub_value)
{
    double v = 0.0;
    if ((int)threadIdx.x < 5) {
        v = gbuf[threadIdx.x];
        for (int r = 1; r < nranks; ++r) v += gbuf[(size_t)r * slot_doubles + threadIdx.x];
        dots_out[threadIdx.x] = v;
    }
    const double2* g2 = reinterpret_cast<const double2*>(gbuf);
    for (int j = threadIdx.x; j < nghost; j += kFinalThreads) rs_ghost[j] = g2[ghost_src[j]];
    if (pub) {
        // the ghost rows are part of what the waiting launch reads after the publication (its boundary tiles):
        // plain stores of every wave drained -> barrier -> agent-scope release -> publication
        // (cdna_hip_programming.md Guideline 16: producer side of the release / acquire form)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (threadIdx.x < 64) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            publish(pub, v, 5, pub_value);
        }
    }
}

// ---- direct peer exchange outside the iteration launches (PeerDev, prcg_kernels.h) ----
__global__ __launch_bounds__(256) void k_peer_push(const PeerDev* __restrict__ px, const double2* __restrict__ rs,
                                                   const double* __restrict__ dots, int k, int contribute) {
    const int R = px->nranks;
    const long long gout = peer_ghost_off(R, px->ghost_cap, k & 1);
    for (int e = threadIdx.x; e < px->n_send; e += 256) {
        const int4 ent = px->send_ent[e];
        const double2 v = rs[ent.x];
        double* dst = px->peer[ent.y] + gout + 2 * (long long)ent.z;
        peer_store(dst, v.x);
        peer_store(dst + 1, v.y);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x < 64) {
        // rank 0 contributes the (global) inner products of state k, the others zeros: added in rank order that is dots
        const double v = (threadIdx.x < 5 && contribute) ? dots[threadIdx.x] : 0.0;
        peer_send_slot(px, k, v);
    }
}
__global__ __launch_bounds__(256) void k_peer_collect(const PeerDev* __restrict__ px, int k, const double* __restrict__ partials, int nparts,
                                                      double* __restrict__ dots_out, double* pub, unsigned* err) {
    __shared__ double s_mine[5];
    if (nparts > 0) {      // the same 256-thread tree as workgroup 0 of a following launch would use
        double mine[5];
        sum_prev_partials<5, 4>(partials, nparts, 0, mine);
        if (threadIdx.x < 5) s_mine[threadIdx.x] = mine[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x >= 64) return;
    const int lane = threadIdx.x;
    double tot[5];
    if (nparts > 0) {
        double v = 0.0;
#pragma unroll
        for (int q = 0; q < 5; ++q) v = lane == q ? s_mine[q] : v;
        peer_send_slot(px, k, v);
    }
    const bool ok = peer_collect(px, k, 1u << 24, tot);
    if (!ok && lane == 0) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < 5; ++q) v = lane == q ? tot[q] : v;
    if (lane < 5 && dots_out) dots_out[lane] = v;
    if (pub) publish(pub, v, 5, (unsigned)k);
}

__global__ __launch_bounds__(64) void k_publish(const double* __restrict__ dots, double* pub, unsigned value) {
    const double v = threadIdx.x < 5 ? dots[threadIdx.x] : 0.0;
    publish(pub, v, 5, value);
}

// ---- utilities -------------------------------------------------------------------------
__global__ void k_copy(double* dst, int ds, const double* src, int ss, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i * ds] = src[i * ss];
}
__global__ void k_sub(double* dst, int ds, const double* a, int as, const double* b, int bs, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i * ds] = a[i * as] - b[i * bs];
}
__global__ void k_mul(double* dst, int ds, const double* a, int as, const double* b, int bs, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        dst[i * ds] = a[i * as] * b[i * bs];
}
__global__ __launch_bounds__(kBlock) void k_diff_sq(const double* __restrict__ a, int as, const double* __restrict__ b,
                                                    int64_t n, double* partials, int slot, int trips) {
    double acc[1] = {0.0};
    int64_t i = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x * 2;
    for (int j = 0; j < trips; ++j, i += kElemsPerTrip) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t ie = i + e;
            if (ie >= n) break;
            const double dlt = a[ie * as] - b[ie];
            acc[0] += dlt * dlt;
        }
    }
    block_reduce_store<1>(acc, partials, slot);
}
__global__ __launch_bounds__(kBlock) void k_dot(const double* __restrict__ a, const double* __restrict__ b, int64_t n,
                                                double* partials, int slot, int trips) {
    double acc[1] = {0.0};
    int64_t i = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x * 2;
    for (int j = 0; j < trips; ++j, i += kElemsPerTrip) {
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t ie = i + e;
            if (ie >= n) break;
            acc[0] += a[ie] * b[ie];
        }
    }
    block_reduce_store<1>(acc, partials, slot);
}
__global__ void k_pack(double* buf, const double* v, const int* idx, int64_t count, int nc) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < count; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t src = idx[j];
        for (int c = 0; c < nc; ++c) buf[j * nc + c] = v[src * nc + c];
    }
}


int util_grid(int64_t n) {
    int64_t g = (n + 255) / 256;
    if (g > 4096) g = 4096;
    if (g < 1) g = 1;
    return (int)g;
}

// Persistent grid for the tile kernels = blocks that are truly co-resident.  The strided
// tile assignment assumes every block runs from the start; a block that has to queue
// behind the others turns into a serial tail (measured: 32 KiB blocks at the occupancy
// API's 5 per CU run 17 % slower than at 4 per CU -- only 4 are resident).  The LDS of a
// CU is handed out per half (80 KiB each), so residency = 2 * floor(80 KiB / block LDS),
// further capped by the API and by 8 blocks (32 waves) per CU.
template <int TAG, typename K>
int tile_grid(K kernel, int ntiles, int per_cu_override) {
    static int caps[16] = {};   // per TAG (the kernels share one function-pointer type) and device
    int devid = 0;
    (void)hipGetDevice(&devid);
    int& cap = caps[devid & 15];
    if (cap == 0) {
        int dev = 0, cus = 256, occ = 4;
        if (hipGetDevice(&dev) == hipSuccess) {
            (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, kBlock, 0) != hipSuccess || occ < 1) occ = 4;
            hipFuncAttributes fa;
            if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kernel)) == hipSuccess && fa.sharedSizeBytes > 0) {
                const int by_lds = 2 * (int)((80 * 1024) / fa.sharedSizeBytes);
                if (by_lds >= 1 && by_lds < occ) occ = by_lds;
            }
            if (occ > 8) occ = 8;
            // Measured on MI355X (profiles/r01_sweeps.md): beyond ~12 resident waves per CU
            // of this two-deep pipeline the extra outstanding streams cost more HBM
            // efficiency than the latency hiding they add (S3: 3 blocks/CU 5.2 TB/s,
            // 4 blocks/CU 4.6 TB/s at 512-slot tiles; 256-slot tiles, which are chosen for
            // short-row operators, likewise: S2 3/CU 3236 it/s vs 4/CU 3065, S1 35.2 k vs 34.1 k).
            // TAG = NV*1000 + EPI*100 + STEPS*10 + (column bytes on the stream: 0 = int32, 1, 2);
            // with the narrower column stream one more resident block pays (S3: 2394 vs 2317 it/s)
            const int steps_ = (TAG / 10) % 10, narrow_ = TAG % 10;
            // (codes 4..6: value dictionary beside int32 / 8-bit / 16-bit columns -- lighter stream, fewer
            //  registers: 4 blocks also at 256-slot tiles, S2 4103 vs 3666 it/s, S1 36.6 k vs 35.4 k)
            const int tuned = steps_ == 4 ? 2 : (((steps_ == 2 && narrow_ != 0) || narrow_ >= 4) ? 4 : 3);
            if (occ > tuned) occ = tuned;
        }
        cap = occ * cus;
    }
    int g = (ntiles + kWaves - 1) / kWaves;
    int lim = cap;
    if (per_cu_override >= 1 && per_cu_override <= 16) {      // experiment knob PRCG_GRID_PER_CU (read into the handle)
        int cus = 256;
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, devid);
        lim = per_cu_override * cus;
    }
    if (g > lim) g = lim;
    if (g < 1) g = 1;
    return g;
}

}  // namespace

// ---- launch wrappers -------------------------------------------------------------------
#define PRCG_LAUNCH_OK() (hipGetLastError() == hipSuccess)

template <int NV, int EPI, int STEPS>
int launch_tiles(hipStream_t st, const CsrDev& A, const Tile* tiles, int ntiles, const void* x, void* y,
                 int write_mask, const double* ep_r, const double* ep_d, double* ep_st, double* partials,
                 TileKnobs kn, double* aux = nullptr, FusedPrev fz = FusedPrev{})
{
    const int cw = A.tile_base == nullptr ? 0 : (A.col8 ? 8 : (A.col16 ? 16 : 0));
    const bool vd = A.vidx8 != nullptr;   // value dictionary
    auto k = cw == 8 ? (vd ? k_spmv_tiles<NV, EPI, STEPS, 8, true> : k_spmv_tiles<NV, EPI, STEPS, 8, false>)
                     : (cw == 16 ? (vd ? k_spmv_tiles<NV, EPI, STEPS, 16, true> : k_spmv_tiles<NV, EPI, STEPS, 16, false>)
                                 : (vd ? k_spmv_tiles<NV, EPI, STEPS, 0, true> : k_spmv_tiles<NV, EPI, STEPS, 0, false>));
    int grid;
    if (cw == 8) grid = vd ? tile_grid<NV * 1000 + EPI * 100 + STEPS * 10 + 5>(k, ntiles, kn.per_cu) : tile_grid<NV * 1000 + EPI * 100 + STEPS * 10 + 1>(k, ntiles, kn.per_cu);
    else if (cw == 16) grid = vd ? tile_grid<NV * 1000 + EPI * 100 + STEPS * 10 + 6>(k, ntiles, kn.per_cu) : tile_grid<NV * 1000 + EPI * 100 + STEPS * 10 + 2>(k, ntiles, kn.per_cu);
    else grid = vd ? tile_grid<NV * 1000 + EPI * 100 + STEPS * 10 + 4>(k, ntiles, kn.per_cu) : tile_grid<NV * 1000 + EPI * 100 + STEPS * 10>(k, ntiles, kn.per_cu);
    hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, st, A, tiles, A.tile_base, A.vd, ntiles, x, y, write_mask, ep_r, ep_d, ep_st,
                       partials, aux, fz);
    return PRCG_LAUNCH_OK() ? grid : -1;
}

template <int NV, int EPI>
int launch_tiles_steps(int steps, hipStream_t st, const CsrDev& A, const Tile* tiles, int ntiles, const void* x,
                       void* y, int write_mask, const double* ep_r, const double* ep_d, double* ep_st,
                       double* partials, TileKnobs kn, double* aux = nullptr, FusedPrev fz = FusedPrev{})
{
    switch (steps) {
    case 1: return launch_tiles<NV, EPI, 1>(st, A, tiles, ntiles, x, y, write_mask, ep_r, ep_d, ep_st, partials, kn, aux, fz);
    case 2: return launch_tiles<NV, EPI, 2>(st, A, tiles, ntiles, x, y, write_mask, ep_r, ep_d, ep_st, partials, kn, aux, fz);
    case 4: return launch_tiles<NV, EPI, 4>(st, A, tiles, ntiles, x, y, write_mask, ep_r, ep_d, ep_st, partials, kn, aux, fz);
    default: return -1;
    }
}

int launch_spmv(hipStream_t st, const CsrDev& A, const Tile* tiles, int ntiles, int steps,
                const double* x, double* y, SpmvEpilogue epi,
                const double* ep_r, const double* ep_d, double* ep_st, double* partials, TileKnobs kn, const StopAt& stop)
{
    if (stop && epi != kEpiDotXY) return -1;
    if (ntiles <= 0) return 0;
    if (stop)
        return launch_tiles_steps<1, kEpiDotXYStop>(steps, st, A, tiles, ntiles, x, y, 3, nullptr, nullptr, nullptr, partials, kn, nullptr,
                                                    product_prev(stop));
    switch (epi) {
    case kEpiNone: return launch_tiles_steps<1, kEpiNone>(steps, st, A, tiles, ntiles, x, y, 3, ep_r, ep_d, ep_st, partials, kn);
    case kEpiDotXY: return launch_tiles_steps<1, kEpiDotXY>(steps, st, A, tiles, ntiles, x, y, 3, ep_r, ep_d, ep_st, partials, kn);
    case kEpiPR: return launch_tiles_steps<1, kEpiPR>(steps, st, A, tiles, ntiles, x, y, 3, ep_r, ep_d, ep_st, partials, kn);
    case kEpiCG: return launch_tiles_steps<1, kEpiCG>(steps, st, A, tiles, ntiles, x, y, 3, ep_r, ep_d, ep_st, partials, kn);
    default: break;
    }
    return -1;
}

int launch_spmm2(hipStream_t st, const CsrDev& A, const Tile* tiles, int ntiles, int steps,
                 const double* rs, double* wu, int write_mask, TileKnobs kn, const StopAt& stop)
{
    if (ntiles <= 0) return 0;
    if (stop)
        return launch_tiles_steps<2, kEpiNoneStop>(steps, st, A, tiles, ntiles, rs, wu, write_mask, nullptr, nullptr, nullptr,
                                                   nullptr, kn, nullptr, product_prev(stop));
    return launch_tiles_steps<2, kEpiNone>(steps, st, A, tiles, ntiles, rs, wu, write_mask, nullptr, nullptr, nullptr,
                                           nullptr, kn);
}

int launch_pipe_fused(hipStream_t st, const CsrDev& A, const Tile* tiles, int ntiles, int steps, const FusedState& f, TileKnobs kn)
{
    if (ntiles <= 0) return 0;
    FusedPrev fz = f.prev;
    fz.rs = f.rs; fz.w = f.w; fz.wt = f.wt;
    const int mask = 3 | (f.meurant ? 4 : 0) | (f.stream_stores ? 8 : 0);
    if (f.dinv) {
        if (f.recompute_w)
            return launch_tiles_steps<2, kEpiPipeFusedJ>(steps, st, A, tiles, ntiles, f.in_old, f.xp, mask, f.dots_prev, f.dinv,
                                                         f.in_new, f.partials, kn, f.coef_out, fz);
        return launch_tiles_steps<2, kEpiPipeFusedPJ>(steps, st, A, tiles, ntiles, f.in_old, f.xp, mask, f.dots_prev, f.dinv,
                                                      f.in_new, f.partials, kn, f.coef_out, fz);
    }
    if (f.recompute_w)
        return launch_tiles_steps<2, kEpiPipeFused>(steps, st, A, tiles, ntiles, f.in_old, f.xp, mask, f.dots_prev, nullptr,
                                                    f.in_new, f.partials, kn, f.coef_out, fz);
    return launch_tiles_steps<2, kEpiPipeFusedP>(steps, st, A, tiles, ntiles, f.in_old, f.xp, mask, f.dots_prev, nullptr,
                                                 f.in_new, f.partials, kn, f.coef_out, fz);
}

int launch_pipe_update(hipStream_t st, const PipeUpdateArgs& a, const StopAt& stop) {
    if (stop && (!a.ut || a.d)) return -1;       // the stop form: the stored-tilde flavour only (u~ and w~ are vectors)
    const Chunking c = chunking(a.n);
    // preconditioned: the inverse diagonal, or u~ / w~ as vectors (host-callback preconditioner)
    if (stop)             hipLaunchKernelGGL(k_pipe_update_stop, dim3(c.grid), dim3(kBlock), 0, st, a, c.trips, stop.word, stop.k);
    else if (a.d || a.ut) hipLaunchKernelGGL((k_pipe_update<true, false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    else                  hipLaunchKernelGGL((k_pipe_update<false, false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}
int launch_pipe_dots(hipStream_t st, const PipeUpdateArgs& a) {
    const Chunking c = chunking(a.n);
    if (a.d || a.ut) hipLaunchKernelGGL((k_pipe_update<true, true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    else             hipLaunchKernelGGL((k_pipe_update<false, true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}

int launch_hs_update_xr(hipStream_t st, const HsArgs& a, const double* prev_mu, int nprev, double* dots_prev_w, const StopAt& stop) {
    if (stop && stop.k < 1) return -1;
    const Chunking c = chunking(a.n);
    if (stop) {
        if (a.d) hipLaunchKernelGGL((k_hs_update_xr_stop<true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips, prev_mu, nprev, dots_prev_w, stop.decides(), stop.k);
        else     hipLaunchKernelGGL((k_hs_update_xr_stop<false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips, prev_mu, nprev, dots_prev_w, stop.decides(), stop.k);
    }
    else if (a.d) hipLaunchKernelGGL((k_hs_update_xr<true, false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips, prev_mu, nprev, dots_prev_w);
    else          hipLaunchKernelGGL((k_hs_update_xr<false, false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips, prev_mu, nprev, dots_prev_w);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}
int launch_hs_init_dots(hipStream_t st, const HsArgs& a) {
    const Chunking c = chunking(a.n);
    const double* none = nullptr;
    double* nonew = nullptr;
    if (a.d) hipLaunchKernelGGL((k_hs_update_xr<true, true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips, none, 0, nonew);
    else     hipLaunchKernelGGL((k_hs_update_xr<false, true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips, none, 0, nonew);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}
int launch_hs_update_p(hipStream_t st, const HsArgs& a, const double* prev_nu, int nprev, double* dots_cur_w, const StopAt& stop) {
    const Chunking c = chunking(a.n);
    if (stop) hipLaunchKernelGGL(k_hs_update_p_stop, dim3(c.grid), dim3(kBlock), 0, st, a, c.trips, prev_nu, nprev, dots_cur_w, stop.word, stop.k);
    else      hipLaunchKernelGGL(k_hs_update_p, dim3(c.grid), dim3(kBlock), 0, st, a, c.trips, prev_nu, nprev, dots_cur_w);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}
void launch_reduce_hs_mu(hipStream_t st, const double* partials, int nparts, double* row, const StopAt& stop) {
    if (stop) hipLaunchKernelGGL(k_reduce_hs_mu_stop, dim3(1), dim3(kFinalThreads), 0, st, partials, nparts, row, stop.decides(), stop.k);
    else      hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(kFinalThreads), 0, st, partials, nparts, row, 0, 0 /* PRCG_S_MU */, 1);
}

int launch_pr_update(hipStream_t st, const PrArgs& a) {
    const Chunking c = chunking(a.n);
    if (a.precond) hipLaunchKernelGGL((k_pr_update<true, false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    else           hipLaunchKernelGGL((k_pr_update<false, false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}
int launch_pr_init_dots(hipStream_t st, const PrArgs& a) {
    const Chunking c = chunking(a.n);
    if (a.precond) hipLaunchKernelGGL((k_pr_update<true, true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    else           hipLaunchKernelGGL((k_pr_update<false, true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}

int launch_cg_update_ps(hipStream_t st, const CgArgs& a, const double* prev, int nprev) {
    const Chunking c = chunking(a.n);
    hipLaunchKernelGGL(k_cg_update_ps, dim3(c.grid), dim3(kBlock), 0, st, a, c.trips, prev, nprev);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}
int launch_gv_update1(hipStream_t st, const CgArgs& a, bool dots_only) {
    const Chunking c = chunking(a.n);
    if (a.rt) {      // preconditioned (a.d null: w~ = M^-1 w is applied by the caller afterwards)
        if (dots_only) hipLaunchKernelGGL((k_gv_update1<true, true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
        else hipLaunchKernelGGL((k_gv_update1<true, false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    } else {
        if (dots_only) hipLaunchKernelGGL((k_gv_update1<false, true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
        else hipLaunchKernelGGL((k_gv_update1<false, false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    }
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}

int launch_reduce_final(hipStream_t st, const double* partials, int nparts, double* out,
                        int src_first, int dst_first, int count, const StopAt& stop) {
    if (stop && (src_first != 0 || dst_first != 0 || count != 5)) return -1;      // the stop form sums and judges a whole pipelined row
    if (stop) hipLaunchKernelGGL(k_reduce_final_stop, dim3(1), dim3(kFinalThreads), 0, st, partials, nparts, out, stop.decides(), stop.k);
    else      hipLaunchKernelGGL(k_reduce_final, dim3(1), dim3(kFinalThreads), 0, st, partials, nparts, out, src_first, dst_first, count);
    return 0;      // (a launch error is left for the next checked launch to report, as ever)
}

void launch_reduce_final_jobs(hipStream_t st, const ReduceJobs& jobs, int njobs) {
    if (njobs < 1 || njobs > kMaxReduceJobs) return;
    hipLaunchKernelGGL(k_reduce_final_jobs, dim3(njobs), dim3(kFinalThreads), 0, st, jobs);
}

void launch_copy(hipStream_t st, double* dst, int ds, const double* src, int ss, int64_t n) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_copy, dim3(util_grid(n)), dim3(256), 0, st, dst, ds, src, ss, n);
}
void launch_sub(hipStream_t st, double* dst, int ds, const double* a, int as, const double* b, int bs, int64_t n) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_sub, dim3(util_grid(n)), dim3(256), 0, st, dst, ds, a, as, b, bs, n);
}
void launch_mul(hipStream_t st, double* dst, int ds, const double* a, int as, const double* b, int bs, int64_t n) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_mul, dim3(util_grid(n)), dim3(256), 0, st, dst, ds, a, as, b, bs, n);
}
int launch_diff_sq(hipStream_t st, const double* a, int as, const double* b, int64_t n, double* partials, int slot) {
    const Chunking c = chunking(n);
    hipLaunchKernelGGL(k_diff_sq, dim3(c.grid), dim3(kBlock), 0, st, a, as, b, n, partials, slot, c.trips);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}
int launch_dot(hipStream_t st, const double* a, const double* b, int64_t n, double* partials, int slot) {
    const Chunking c = chunking(n);
    hipLaunchKernelGGL(k_dot, dim3(c.grid), dim3(kBlock), 0, st, a, b, n, partials, slot, c.trips);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}
void launch_gather_pack(hipStream_t st, const double* partials, int nparts, double* slot, const double* rs,
                        const int* send_idx, int nsend) {
    hipLaunchKernelGGL(k_gather_pack, dim3(1), dim3(kFinalThreads), 0, st, partials, nparts, slot,
                       reinterpret_cast<const double2*>(rs), send_idx, nsend);
}
void launch_gather_unpack(hipStream_t st, const double* gbuf, int slot_doubles, int nranks, double* dots_out,
                          double* rs_ghost, const int* ghost_src, int nghost, double* pub, unsigned pub_value, hipEvent_t done) {
    if (done)      // the launch's own completion signal (no marker packet behind it)
        hipExtLaunchKernelGGL(k_gather_unpack, dim3(1), dim3(kFinalThreads), 0, st, nullptr, done, 0, gbuf, slot_doubles, nranks,
                              dots_out, reinterpret_cast<double2*>(rs_ghost), ghost_src, nghost, pub, pub_value);
    else
        hipLaunchKernelGGL(k_gather_unpack, dim3(1), dim3(kFinalThreads), 0, st, gbuf, slot_doubles, nranks, dots_out,
                           reinterpret_cast<double2*>(rs_ghost), ghost_src, nghost, pub, pub_value);
}
// One wave that waits (bounded, ~2 ms) for copy 0 of a publication record to reach `want`: the probe
// prcg_solve_begin uses to find out whether a kernel of the communication stream can run WHILE a kernel of
// the compute stream waits for it (two HIP streams may share one hardware queue, which is in order).
__global__ __launch_bounds__(64) void k_probe_wait(const double* pub, unsigned want, unsigned* err) {
    const unsigned* cnt = reinterpret_cast<const unsigned*>(pub + 6);
    unsigned spins = 0;
    bool ok = false;
    while (!(ok = (int)(__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - want) >= 0) && ++spins < 4096u)
        __builtin_amdgcn_s_sleep(16);
    if (!ok && threadIdx.x == 0) __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// ---- what the memory system delivers for the iteration's own byte mix (bench.py: roofline.stream_ceiling_GBps) ----
// mode 0: pure 16-byte-per-lane read (8 loads in flight per thread); mode 1 / 2: per row one pair read and rewritten in
// place, one pair read from one array and written to another -- 2 x 16 B in, 2 x 16 B out, the vector traffic of the
// one-launch pipelined iteration with nothing else -- with plain (1) or nontemporal (2) stores.
template <int UNROLL>
__global__ __launch_bounds__(256) void k_stream_read(const double2* __restrict__ a, size_t n2, double* out) {
    double s = 0.0;
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i + (UNROLL - 1) * stride < n2; i += UNROLL * stride) {
        double2 v[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) v[u] = a[i + u * stride];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) s += v[u].x + v[u].y;
    }
    for (; i < n2; i += stride) { const double2 v = a[i]; s += v.x + v.y; }
    if (s == 123.456) out[0] = s;                                           // (keeps the loads alive)
}
template <int UNROLL, bool NT>
__global__ __launch_bounds__(256) void k_stream_pairs(double2* __restrict__ xp, const double2* __restrict__ rs, double2* __restrict__ rsn, size_t n2) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    typedef double d2 __attribute__((ext_vector_type(2)));
    d2* X = reinterpret_cast<d2*>(xp);
    const d2* R = reinterpret_cast<const d2*>(rs);
    d2* Rn = reinterpret_cast<d2*>(rsn);
    for (; i < n2; i += UNROLL * stride) {
        d2 x[UNROLL], r[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) if (i + u * stride < n2) { x[u] = X[i + u * stride]; r[u] = R[i + u * stride]; }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) if (i + u * stride < n2) {
            const d2 xo = x[u], ro = r[u];
            const d2 xn = {xo.x + 0.5 * xo.y, ro.x + 0.25 * xo.y}, rn = {ro.x - 0.5 * ro.y, xo.y + 0.25 * ro.y};
            if (NT) { __builtin_nontemporal_store(xn, X + i + u * stride); __builtin_nontemporal_store(rn, Rn + i + u * stride); }
            else { X[i + u * stride] = xn; Rn[i + u * stride] = rn; }
        }
    }
}
// pure read as a streaming kernel should issue it (tools/readpat.hip: 6.5-7.1 TB/s where the grid-stride form above with eight
// 1 KB pieces per wave in flight and 16+ waves per CU reads 5.1-5.5): every wave walks contiguous 4 KB chunks, four nontemporal
// 16-byte loads in flight, eight waves per CU
__global__ __launch_bounds__(256) void k_stream_read_chunks(const double2* __restrict__ a_, size_t n2, double* out) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const d2* a = reinterpret_cast<const d2*>(a_);
    const int lane = threadIdx.x & 63;
    const size_t W = (size_t)gridDim.x * 4, w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const size_t chunks = n2 / 256;                                          // 256 pairs = 4 KB
    double s = 0.0;
    for (size_t c = w; c < chunks; c += W) {
        const d2* base = a + c * 256 + lane;
        d2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = __builtin_nontemporal_load(base + u * 64);
#pragma unroll
        for (int u = 0; u < 4; ++u) s += v[u].x + v[u].y;
    }
    if (s == 123.456) out[0] = s;
}
// the byte MIX of a one-launch iteration with no arithmetic to speak of (tools/mixbench.hip): per piece of 64 rows a wave reads
// `kb` KB of an operator stream (nontemporal, read once: 16 one-KB loads in flight, the next 16 requested before these are used),
// reads the rows' two pairs and writes one in place and one to another array with nontemporal stores.  What the memory system
// delivers for THIS mix is the ceiling of a kernel that moves it: 0.32 GB of row results beside a 1.3 GB stream cost 55-90 us
// (read / write turnarounds), beside a 3 GB stream 76 us -- in the mix itself, not in the kernel.
__global__ __launch_bounds__(256) void k_stream_mix(const double2* __restrict__ V_, double2* __restrict__ X_, const double2* __restrict__ R_,
                                                    double2* __restrict__ Rn_, size_t n_rows, int kb) {
    typedef double d2 __attribute__((ext_vector_type(2)));
    const d2* V = reinterpret_cast<const d2*>(V_);
    d2* X = reinterpret_cast<d2*>(X_);
    const d2* R = reinterpret_cast<const d2*>(R_);
    d2* Rn = reinterpret_cast<d2*>(Rn_);
    const int lane = threadIdx.x & 63;
    const size_t W = (size_t)gridDim.x * 4, w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const size_t pieces = n_rows / 64;
    constexpr int CH = 16;
    const int nch = (kb + CH - 1) / CH;
    for (size_t p = w; p < pieces; p += W) {
        const d2* base = V + p * (size_t)kb * 64 + lane;
        const d2 x = X[p * 64 + lane], r = R[p * 64 + lane];
        d2 a[CH], b[CH];
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < CH; ++u) a[u] = __builtin_nontemporal_load(base + (size_t)(u < kb ? u : 0) * 64);
        for (int c = 1; c <= nch; ++c) {
            if (c < nch) {
#pragma unroll
                for (int u = 0; u < CH; ++u) { const int q = c * CH + u; b[u] = __builtin_nontemporal_load(base + (size_t)(q < kb ? q : 0) * 64); }
            }
#pragma unroll
            for (int u = 0; u < CH; ++u) s += a[u].x + a[u].y;
#pragma unroll
            for (int u = 0; u < CH; ++u) a[u] = b[u];
        }
        const d2 xn = {x.x + 0.5 * x.y + s, r.x + 0.25 * x.y}, rn = {r.x - 0.5 * r.y, x.y + 0.25 * r.y};
        __builtin_nontemporal_store(xn, X + p * 64 + lane);
        __builtin_nontemporal_store(rn, Rn + p * 64 + lane);
    }
}
void launch_stream_mix(hipStream_t st, const double* v, double* x, const double* r, double* rn, size_t n_rows, int kb) {
    hipLaunchKernelGGL(k_stream_mix, dim3(512), dim3(256), 0, st, reinterpret_cast<const double2*>(v), reinterpret_cast<double2*>(x),
                       reinterpret_cast<const double2*>(r), reinterpret_cast<double2*>(rn), n_rows, kb);
}
void launch_stream_probe(hipStream_t st, int mode, double* a, double* b, double* c, size_t n_pairs) {
    const dim3 grid(kMaxGridBlocks), block(256);
    if (mode == 3) { hipLaunchKernelGGL(k_stream_read_chunks, dim3(512), block, 0, st, reinterpret_cast<const double2*>(a), n_pairs, c); return; }
    if (mode == 0) hipLaunchKernelGGL(k_stream_read<8>, grid, block, 0, st, reinterpret_cast<const double2*>(a), n_pairs, c);
    else if (mode == 1) hipLaunchKernelGGL((k_stream_pairs<4, false>), grid, block, 0, st, reinterpret_cast<double2*>(a), reinterpret_cast<const double2*>(b), reinterpret_cast<double2*>(c), n_pairs);
    else hipLaunchKernelGGL((k_stream_pairs<4, true>), grid, block, 0, st, reinterpret_cast<double2*>(a), reinterpret_cast<const double2*>(b), reinterpret_cast<double2*>(c), n_pairs);
}

void launch_probe_wait(hipStream_t st, const double* pub, unsigned want, unsigned* err) {
    hipLaunchKernelGGL(k_probe_wait, dim3(1), dim3(64), 0, st, pub, want, err);
}

// bit 30 of a window tile's `geo` word: some of its rows go to neighbours (the iteration launch then looks at tile_send)
__global__ void k_flag_send_tiles(int* __restrict__ wtiles, const int2* __restrict__ tile_send, int ntiles) {
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < ntiles; t += gridDim.x * blockDim.x) {
        const int2 ts = tile_send[t];
        int& geo = wtiles[(size_t)t * 24 + 4];
        geo = ts.y > ts.x ? (geo | (1 << 30)) : (geo & ~(1 << 30));
    }
}
void launch_flag_send_tiles(hipStream_t st, void* wtiles, const void* tile_send, int ntiles) {
    if (ntiles > 0) hipLaunchKernelGGL(k_flag_send_tiles, dim3((ntiles + 255) / 256), dim3(256), 0, st, static_cast<int*>(wtiles), static_cast<const int2*>(tile_send), ntiles);
}
void launch_peer_push(hipStream_t st, const PeerDev* px, const double* rs, const double* dots, int k, int contribute) {
    hipLaunchKernelGGL(k_peer_push, dim3(1), dim3(256), 0, st, px, reinterpret_cast<const double2*>(rs), dots, k, contribute);
}
void launch_peer_collect(hipStream_t st, const PeerDev* px, int k, const double* partials, int nparts, double* dots_out, double* pub,
                         unsigned* err) {
    hipLaunchKernelGGL(k_peer_collect, dim3(1), dim3(256), 0, st, px, k, partials, nparts, dots_out, pub, err);
}
void launch_publish(hipStream_t st, const double* dots, double* pub, unsigned value) {
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, st, dots, pub, value);
}
void launch_pack(hipStream_t st, double* buf, const double* v, const int* idx, int64_t count, int nc) {
    if (count <= 0) return;
    hipLaunchKernelGGL(k_pack, dim3(util_grid(count)), dim3(256), 0, st, buf, v, idx, count, nc);
}

}  // namespace prcg
