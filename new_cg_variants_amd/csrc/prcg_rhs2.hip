// gfx950 (MI355X / CDNA4): the vector kernels of the session type "Hestenes-Stiefel, two right-hand sides"
// (prcg_solve_begin_multi; replaces two calls of the reference's hs_cg.py:9 / :70 on one matrix), and below them those of
// "predict-and-recompute, two right-hand sides" (pr_cg.py:166 / :172; k_pr2_*) and of "pipelined predict-and-recompute, two
// right-hand sides" (prcg_solve_begin_multi_pipe; pipe_pr_cg.py:89 / :201 / :101 / :213; k_pipe2_update).
//
// One iteration of the session is  update_xr -> reduce -> update_p -> [p_0 p_1] -> A [p_0 p_1] (the two-vector product
// every operator family already has) -> dot_ps -> reduce: the operator is streamed ONCE for both systems.
//
// State layout: X, R, P, S (and RT with Jacobi) are interleaved n x 2 arrays, row i = (column 0, column 1).  A lane touches
// a row of an array with ONE 16-byte load or store, a wave instruction covers one contiguous kilobyte, and P / S are
// directly the product's input and output.  All three kernels are bandwidth bound: per row update_xr moves 96 bytes
// (x, r, p, s in; x, r out; + 8 of d in and 16 of rt out with Jacobi), update_p 48, dot_ps 32.
//
// Arithmetic: the expressions of k_hs_update_xr / k_hs_update_p (prcg_kernels.hip), multiply then add, every product
// and every sum rounded (-ffp-contract=off).  Each column has its OWN scalars (a_c, b_c, its own accumulators): nothing
// one column computes enters the other, there is no branch on a value and no 0 * x shortcut -- a NaN or inf of one
// system stays in that system, and swapping the right-hand sides swaps the results bit for bit.
//
// Order of the sums (what tests/device_order.py: device_sum models, so the oracle can be asked for equal bits): grid and
// trips as chunking(n); thread t of block b adds elements (b * trips + j) * 512 + t, then + 256 + t, for ascending j;
// xor butterfly per wave; waves 0..3 in order (block_reduce_store); the block partials by launch_reduce_final.
#include <hip/hip_runtime.h>

#include "prcg_kernels.h"
#include "prcg_device.hpp"

namespace prcg {
namespace {

// a_c = nu_c / mu_c; x += a_c p; r -= a_c s; (z = d r); partials of nu_c = r.z and rr_c = r.r   (hs_cg.py:54-56, hs_pcg :116-119)
template <bool PREC, bool DOTS_ONLY>
__global__ __launch_bounds__(kBlock) void k_hs2_update_xr(Hs2Args a, int trips) {
    double al0 = 0.0, al1 = 0.0;
    if constexpr (!DOTS_ONLY) {
        const double* __restrict__ dp = a.dots_prev;
        al0 = dp[kHs2Nu] / dp[kHs2Mu];                          // a_k1 = nu / mu, column 0
        al1 = dp[kHs2Nu + 2] / dp[kHs2Mu + 1];                  // ... column 1
        if (blockIdx.x == 0 && threadIdx.x == 0) { a.coef_out[0] = al0; a.coef_out[2] = al1; }
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};                       // nu_0, rr_0, nu_1, rr_1
    const int64_t n = a.n;
    double2* __restrict__ X = reinterpret_cast<double2*>(a.x);
    double2* __restrict__ R = reinterpret_cast<double2*>(a.r);
    double2* __restrict__ RT = reinterpret_cast<double2*>(a.rt);
    const double2* __restrict__ P = reinterpret_cast<const double2*>(a.p);
    const double2* __restrict__ S = reinterpret_cast<const double2*>(a.s);
    const double* __restrict__ D = a.d;

    int64_t base = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x;
    for (int j = 0; j < trips; ++j, base += kElemsPerTrip) {
        if (base >= n) break;
        // ---- loads of both rows first (two independent rows in flight) ----
        double2 x2[2], r2[2], p2[2], s2[2];
        double dv[2];
        bool ok[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t ie = base + e * kBlock;
            ok[e] = ie < n;
            const int64_t il = ok[e] ? ie : base;               // clamped: branch-free loads
            r2[e] = R[il];
            if constexpr (!DOTS_ONLY) { x2[e] = X[il]; p2[e] = P[il]; s2[e] = S[il]; }
            if constexpr (PREC) dv[e] = D[il];
        }
        // ---- arithmetic + stores, row base then row base + 256 (this order is part of the reduction tree) ----
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (!ok[e]) continue;
            const int64_t ie = base + e * kBlock;
            double2 rn = r2[e];
            if constexpr (!DOTS_ONLY) {
                X[ie] = make_double2(x2[e].x + al0 * p2[e].x, x2[e].y + al1 * p2[e].y);      // x += a p
                rn = make_double2(rn.x - al0 * s2[e].x, rn.y - al1 * s2[e].y);               // r -= a s
                R[ie] = rn;
            }
            if constexpr (PREC) {
                const double2 z = make_double2(dv[e] * rn.x, dv[e] * rn.y);                  // r~ = M^-1 r
                RT[ie] = z;
                acc[0] += rn.x * z.x; acc[1] += rn.x * rn.x;
                acc[2] += rn.y * z.y; acc[3] += rn.y * rn.y;
            } else {
                acc[0] += rn.x * rn.x;
                acc[2] += rn.y * rn.y;
            }
        }
    }
    if constexpr (!PREC) { acc[1] = acc[0]; acc[3] = acc[2]; }
    block_reduce_store<4>(acc, a.partials, kHs2Nu);
}

// b_c = nu_c / nu_prev_c; p = z + b_c p   (hs_cg.py:57-58, hs_pcg :120-121)
__global__ __launch_bounds__(kBlock) void k_hs2_update_p(Hs2Args a, int trips) {
    const double bt0 = a.dots_cur[kHs2Nu] / a.dots_prev[kHs2Nu];            // b_k = nu_k / nu_k1, column 0
    const double bt1 = a.dots_cur[kHs2Nu + 2] / a.dots_prev[kHs2Nu + 2];    // ... column 1
    if (blockIdx.x == 0 && threadIdx.x == 0) { a.coef_out[1] = bt0; a.coef_out[3] = bt1; }
    const int64_t n = a.n;
    const double2* __restrict__ Z = reinterpret_cast<const double2*>(a.rt ? a.rt : a.r);
    double2* __restrict__ P = reinterpret_cast<double2*>(a.p);
    int64_t base = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x;
    for (int j = 0; j < trips; ++j, base += kElemsPerTrip) {
        if (base >= n) break;
        double2 z2[2], p2[2];
        bool ok[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t ie = base + e * kBlock;
            ok[e] = ie < n;
            const int64_t il = ok[e] ? ie : base;
            z2[e] = Z[il]; p2[e] = P[il];
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (!ok[e]) continue;
            P[base + e * kBlock] = make_double2(z2[e].x + bt0 * p2[e].x, z2[e].y + bt1 * p2[e].y);
        }
    }
}

// partials of mu_c = p.s   (hs_cg.py:60): the two-vector products have no dot epilogue
__global__ __launch_bounds__(kBlock) void k_hs2_dot_ps(Hs2Args a, int trips) {
    double acc[2] = {0.0, 0.0};                                 // mu_0, mu_1
    const int64_t n = a.n;
    const double2* __restrict__ P = reinterpret_cast<const double2*>(a.p);
    const double2* __restrict__ S = reinterpret_cast<const double2*>(a.s);
    int64_t base = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x;
    for (int j = 0; j < trips; ++j, base += kElemsPerTrip) {
        if (base >= n) break;
        double2 p2[2], s2[2];
        bool ok[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t ie = base + e * kBlock;
            ok[e] = ie < n;
            const int64_t il = ok[e] ? ie : base;
            p2[e] = P[il]; s2[e] = S[il];
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (!ok[e]) continue;
            acc[0] += p2[e].x * s2[e].x;
            acc[1] += p2[e].y * s2[e].y;
        }
    }
    block_reduce_store<2>(acc, a.partials, kHs2Mu);
}

// ---- predict-and-recompute (pr_cg.py:166 pr_pcg, :172 m_pcg; identity-preconditioned: pr_cg / m_cg), two right-hand sides ----
// One iteration is  update -> [p_0 p_1] -> A [p_0 p_1] -> dots -> two reductions (one per column): ONE reduction point.
// Column c's five sums of iteration k are row 2 k + c of the scalar array in the single-session order [mu dl gm nu rr],
// so predict() serves each column as it serves a single session; the block partials of column c go to part[c] in the
// same slots (the update fills 3..4, the dots kernel 0..2) and one launch_reduce_final per column sums all five.

// (a_c, b_c) = predict(column c's sums of k - 1); x += a p; r -= a s; r~ -= a s~ (without Jacobi r~ IS the new r);
// p = r~ + b p; partials of nu_c = r~.r and rr_c = r.r   (pr_cg.py:146-151, :157)
// DOTS_ONLY, the initial state: (r~ = d r); nu_c, rr_c   (:107-109)
template <bool PREC, bool DOTS_ONLY>
__global__ __launch_bounds__(kBlock) void k_pr2_update(Pr2Args a, int trips) {
    Coefs c0 = {0.0, 0.0, 0.0}, c1 = {0.0, 0.0, 0.0};
    if constexpr (!DOTS_ONLY) {
        c0 = predict(a.dots_prev, a.meurant);
        c1 = predict(a.dots_prev + kPartialStride, a.meurant);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            a.coef_out[0] = c0.al; a.coef_out[1] = c0.bt; a.coef_out[2] = c0.nup;
            a.coef_out[kPr2CoefStride] = c1.al; a.coef_out[kPr2CoefStride + 1] = c1.bt; a.coef_out[kPr2CoefStride + 2] = c1.nup;
        }
    }
    double acc[4] = {0.0, 0.0, 0.0, 0.0};                       // nu_0, rr_0, nu_1, rr_1
    const int64_t n = a.n;
    double2* __restrict__ X = reinterpret_cast<double2*>(a.x);
    double2* __restrict__ R = reinterpret_cast<double2*>(a.r);
    double2* __restrict__ RT = reinterpret_cast<double2*>(a.rt);
    double2* __restrict__ P = reinterpret_cast<double2*>(a.p);
    const double2* __restrict__ S = reinterpret_cast<const double2*>(a.s);
    const double2* __restrict__ ST = reinterpret_cast<const double2*>(a.st);
    const double* __restrict__ D = a.d;

    int64_t base = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x;
    for (int j = 0; j < trips; ++j, base += kElemsPerTrip) {
        if (base >= n) break;
        // ---- loads of both rows first (two independent rows in flight) ----
        double2 x2[2], r2[2], rt2[2], p2[2], s2[2], st2[2];
        double dv[2];
        bool ok[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t ie = base + e * kBlock;
            ok[e] = ie < n;
            const int64_t il = ok[e] ? ie : base;               // clamped: branch-free loads
            r2[e] = R[il];
            if constexpr (!DOTS_ONLY) {
                x2[e] = X[il]; p2[e] = P[il]; s2[e] = S[il];
                if constexpr (PREC) { rt2[e] = RT[il]; st2[e] = ST[il]; }
            } else if constexpr (PREC) {
                dv[e] = D[il];
            }
        }
        // ---- arithmetic + stores, row base then row base + 256 (this order is part of the reduction tree) ----
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (!ok[e]) continue;
            const int64_t ie = base + e * kBlock;
            double2 rn = r2[e], zn;
            if constexpr (!DOTS_ONLY) {
                X[ie] = make_double2(x2[e].x + c0.al * p2[e].x, x2[e].y + c1.al * p2[e].y);  // x += a p
                rn = make_double2(rn.x - c0.al * s2[e].x, rn.y - c1.al * s2[e].y);           // r -= a s
                R[ie] = rn;
                if constexpr (PREC) {
                    zn = make_double2(rt2[e].x - c0.al * st2[e].x, rt2[e].y - c1.al * st2[e].y);   // r~ -= a s~
                    RT[ie] = zn;
                } else {
                    zn = rn;
                }
                P[ie] = make_double2(zn.x + c0.bt * p2[e].x, zn.y + c1.bt * p2[e].y);        // p = r~ + b p
            } else if constexpr (PREC) {
                zn = make_double2(dv[e] * rn.x, dv[e] * rn.y);                               // r~ = M^-1 r
                RT[ie] = zn;
            } else {
                zn = rn;
            }
            acc[0] += zn.x * rn.x; acc[1] += rn.x * rn.x;
            acc[2] += zn.y * rn.y; acc[3] += rn.y * rn.y;
        }
    }
    block_reduce_store2<2>(acc, a.part0, a.part1, kPr2Nu);
}

// after s = A p of both columns: (s~ = d s); partials of mu_c = p.s, dl_c = r.s~, gm_c = s~.s   (pr_cg.py:153-156)
template <bool PREC>
__global__ __launch_bounds__(kBlock) void k_pr2_dots(Pr2Args a, int trips) {
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};             // mu_0, dl_0, gm_0, mu_1, dl_1, gm_1
    const int64_t n = a.n;
    const double2* __restrict__ R = reinterpret_cast<const double2*>(a.r);
    const double2* __restrict__ P = reinterpret_cast<const double2*>(a.p);
    const double2* __restrict__ S = reinterpret_cast<const double2*>(a.s);
    double2* __restrict__ ST = reinterpret_cast<double2*>(a.st);
    const double* __restrict__ D = a.d;
    int64_t base = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x;
    for (int j = 0; j < trips; ++j, base += kElemsPerTrip) {
        if (base >= n) break;
        double2 r2[2], p2[2], s2[2];
        double dv[2];
        bool ok[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t ie = base + e * kBlock;
            ok[e] = ie < n;
            const int64_t il = ok[e] ? ie : base;
            r2[e] = R[il]; p2[e] = P[il]; s2[e] = S[il];
            if constexpr (PREC) dv[e] = D[il];
        }
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (!ok[e]) continue;
            double2 zs = s2[e];
            if constexpr (PREC) {
                zs = make_double2(dv[e] * s2[e].x, dv[e] * s2[e].y);                         // s~ = M^-1 s
                ST[base + e * kBlock] = zs;
            }
            acc[0] += p2[e].x * s2[e].x; acc[1] += r2[e].x * zs.x; acc[2] += zs.x * s2[e].x;
            acc[3] += p2[e].y * s2[e].y; acc[4] += r2[e].y * zs.y; acc[5] += zs.y * s2[e].y;
        }
    }
    block_reduce_store2<3>(acc, a.part0, a.part1, kPr2Mu);
}

// ---- pipelined predict-and-recompute (pipe_pr_cg.py:89 pipe_pr_cg, :101 pipe_pr_m_cg, :201 / :213 with Jacobi), two right-hand sides ----
// One iteration is  update (this kernel, BOTH columns) -> one reduction per column -> [w_0 u_0 | w_1 u_1] = A [r_0 s_0 | r_1 s_1],
// the four-vector product.  The state is NOT interleaved across columns: each column keeps the 16-byte pairs of the single
// session, XP_c = (x,p), RS_c = (r,s), WU_c = (w,u), with Jacobi RSt_c = (r~,s~) -- RS_c (RSt_c) and WU_c are, as they stand, a
// source and a destination pair array of the four-vector product.  Only the flavours that recompute w exist here: WU is
// read and never written, w~ = d w and u~ = d u are formed in registers.
//
// Per row and column the expressions of k_pipe_update (prcg_kernels.hip) in its order, multiply then add; column c has its own
// Coefs and its own five accumulators [mu dl gm nu rr]; a thread's twelve 16-byte loads (two rows x two columns x three arrays;
// sixteen with Jacobi, and two of d) are issued before any arithmetic.  Sums: the tree described at the head of this file.
//
// STOP (k_pipe2_update_stop; a session whose columns stop at their own thresholds, prcg_set_stop_rhs): `words` holds the columns' stop
// words, column c's at words + 2 c.  The reduction that ended an earlier iteration wrote them (k_reduce_final_stop), so they were
// complete before this launch began: every wave reads the same two values through readfirstlane and `live[c]` is a scalar.  A
// column that has stopped is FROZEN -- the launch skips it on scalar branches: no scalar row read, no coefficient row, no load,
// no store, no partial row -- and with both frozen the kernel returns here, before anything else.  The living column executes
// the statements below in their order: its expressions, its accumulators and its tree are those of the kernel without STOP.
template <bool PREC, bool DOTS_ONLY, bool STOP>
__device__ __forceinline__ void pipe2_update_body(const Pipe2Args& a, int trips, const int* __restrict__ words) {
    bool live[2] = {true, true};
    if constexpr (STOP) {
        live[0] = __builtin_amdgcn_readfirstlane(words[0]) < 0;
        live[1] = __builtin_amdgcn_readfirstlane(words[2]) < 0;
        if (!live[0] && !live[1]) return;
    }
    Coefs cf[2] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
    if constexpr (!DOTS_ONLY) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            if (STOP && !live[c]) continue;
            cf[c] = predict(a.dots_prev + c * kPartialStride, a.meurant);
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (STOP && !live[c]) continue;
                double* co = a.coef_out + c * kPr2CoefStride;
                co[0] = cf[c].al; co[1] = cf[c].bt; co[2] = cf[c].nup;
            }
        }
    }
    double acc[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // column 0's mu, dl, gm, nu, rr; column 1's
    const int64_t n = a.n;
    double2* __restrict__ XP[2] = {reinterpret_cast<double2*>(a.xp[0]), reinterpret_cast<double2*>(a.xp[1])};
    double2* __restrict__ RS[2] = {reinterpret_cast<double2*>(a.rs[0]), reinterpret_cast<double2*>(a.rs[1])};
    double2* __restrict__ RST[2] = {reinterpret_cast<double2*>(a.rst[0]), reinterpret_cast<double2*>(a.rst[1])};
    const double2* __restrict__ WU[2] = {reinterpret_cast<const double2*>(a.wu[0]), reinterpret_cast<const double2*>(a.wu[1])};
    const double* __restrict__ D = a.d;

    int64_t base = ((int64_t)blockIdx.x * trips) * kElemsPerTrip + threadIdx.x;
    for (int j = 0; j < trips; ++j, base += kElemsPerTrip) {
        if (base >= n) break;
        // ---- loads of both rows of both columns first ----
        double2 xp[2][2], rs[2][2], wu[2][2], rst[2][2];
        double dv[2];
        bool ok[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int64_t ie = base + e * kBlock;
            ok[e] = ie < n;
            const int64_t il = ok[e] ? ie : base;               // clamped: branch-free loads
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (STOP && !live[c]) continue;                 // scalar branch: a frozen column is not loaded
                xp[c][e] = XP[c][il];
                rs[c][e] = RS[c][il];
                if constexpr (!DOTS_ONLY) wu[c][e] = WU[c][il];
                if constexpr (PREC) rst[c][e] = RST[c][il];
            }
            if constexpr (PREC && !DOTS_ONLY) dv[e] = D[il];
        }
        // ---- arithmetic + stores, row base then row base + 256 (this order is part of the reduction tree) ----
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            if (!ok[e]) continue;
            const int64_t ie = base + e * kBlock;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (STOP && !live[c]) continue;                 // ... nor updated, nor stored
                double* ac = acc + 5 * c;
                const double2 xpv = xp[c][e], rsv = rs[c][e];
                if constexpr (DOTS_ONLY) {
                    if constexpr (PREC) {
                        const double2 rstv = rst[c][e];
                        ac[0] += xpv.y * rsv.y; ac[1] += rsv.x * rstv.y; ac[2] += rstv.y * rsv.y;
                        ac[3] += rstv.x * rsv.x; ac[4] += rsv.x * rsv.x;
                    } else {
                        ac[0] += xpv.y * rsv.y; ac[1] += rsv.x * rsv.y; ac[2] += rsv.y * rsv.y;
                        ac[3] += rsv.x * rsv.x;
                    }
                } else {
                    const double al = cf[c].al, bt = cf[c].bt;
                    const double2 wuv = wu[c][e];
                    const double xn = xpv.x + al * xpv.y;               // x += a p
                    const double rn = rsv.x - al * rsv.y;               // r -= a s
                    const double wn = wuv.x - al * wuv.y;               // w -= a u
                    if constexpr (PREC) {
                        const double2 rstv = rst[c][e];
                        const double ut = dv[e] * wuv.y;                // u~ = M^-1 u
                        const double wtv = dv[e] * wuv.x;               // w~ = M^-1 w
                        const double rtn = rstv.x - al * rstv.y;        // r~ -= a s~
                        const double wtn = wtv - al * ut;               // w~ -= a u~
                        const double pn = rtn + bt * xpv.y;             // p = r~ + b p
                        const double sn = wn + bt * rsv.y;              // s = w + b s
                        const double stn = wtn + bt * rstv.y;           // s~ = w~ + b s~
                        XP[c][ie] = make_double2(xn, pn);
                        RS[c][ie] = make_double2(rn, sn);
                        RST[c][ie] = make_double2(rtn, stn);
                        ac[0] += pn * sn; ac[1] += rn * stn; ac[2] += stn * sn;
                        ac[3] += rtn * rn; ac[4] += rn * rn;
                    } else {
                        const double pn = rn + bt * xpv.y;              // p = r + b p
                        const double sn = wn + bt * rsv.y;              // s = w + b s
                        XP[c][ie] = make_double2(xn, pn);
                        RS[c][ie] = make_double2(rn, sn);
                        ac[0] += pn * sn; ac[1] += rn * sn; ac[2] += sn * sn; ac[3] += rn * rn;
                    }
                }
            }
        }
    }
    if constexpr (!PREC) { acc[4] = acc[3]; acc[9] = acc[8]; }      // unpreconditioned: rr IS nu
    if constexpr (STOP) block_reduce_store2_live<5>(acc, a.part0, a.part1, 0, live);
    else block_reduce_store2<5>(acc, a.part0, a.part1, 0);
}
template <bool PREC, bool DOTS_ONLY>
__global__ __launch_bounds__(kBlock) void k_pipe2_update(Pipe2Args a, int trips) { pipe2_update_body<PREC, DOTS_ONLY, false>(a, trips, nullptr); }
template <bool PREC>
__global__ __launch_bounds__(kBlock) void k_pipe2_update_stop(Pipe2Args a, int trips, const int* __restrict__ words) {
    pipe2_update_body<PREC, false, true>(a, trips, words);
}

}  // namespace

#define PRCG_LAUNCH_OK() (hipGetLastError() == hipSuccess)

int launch_hs2_update_xr(hipStream_t st, const Hs2Args& a) {
    const Chunking c = chunking(a.n);
    if (a.d) hipLaunchKernelGGL((k_hs2_update_xr<true, false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    else     hipLaunchKernelGGL((k_hs2_update_xr<false, false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}
int launch_hs2_init_dots(hipStream_t st, const Hs2Args& a) {
    const Chunking c = chunking(a.n);
    if (a.d) hipLaunchKernelGGL((k_hs2_update_xr<true, true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    else     hipLaunchKernelGGL((k_hs2_update_xr<false, true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}
int launch_hs2_update_p(hipStream_t st, const Hs2Args& a) {
    const Chunking c = chunking(a.n);
    hipLaunchKernelGGL(k_hs2_update_p, dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}
int launch_hs2_dot_ps(hipStream_t st, const Hs2Args& a) {
    const Chunking c = chunking(a.n);
    hipLaunchKernelGGL(k_hs2_dot_ps, dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}

int launch_pr2_update(hipStream_t st, const Pr2Args& a) {
    const Chunking c = chunking(a.n);
    if (a.d) hipLaunchKernelGGL((k_pr2_update<true, false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    else     hipLaunchKernelGGL((k_pr2_update<false, false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}
int launch_pr2_update_stored(hipStream_t st, const Pr2Args& a) {
    const Chunking c = chunking(a.n);
    hipLaunchKernelGGL((k_pr2_update<true, false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}
int launch_pr2_init_dots(hipStream_t st, const Pr2Args& a) {
    const Chunking c = chunking(a.n);
    if (a.d) hipLaunchKernelGGL((k_pr2_update<true, true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    else     hipLaunchKernelGGL((k_pr2_update<false, true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}
int launch_pr2_dots(hipStream_t st, const Pr2Args& a) {
    const Chunking c = chunking(a.n);
    if (a.d) hipLaunchKernelGGL((k_pr2_dots<true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    else     hipLaunchKernelGGL((k_pr2_dots<false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}

int launch_pipe2_update(hipStream_t st, const Pipe2Args& a, const StopAt& stop) {
    const Chunking c = chunking(a.n);
    if (stop) {
        if (a.d) hipLaunchKernelGGL((k_pipe2_update_stop<true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips, stop.word);
        else     hipLaunchKernelGGL((k_pipe2_update_stop<false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips, stop.word);
    }
    else if (a.d) hipLaunchKernelGGL((k_pipe2_update<true, false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    else          hipLaunchKernelGGL((k_pipe2_update<false, false>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}
int launch_pipe2_dots(hipStream_t st, const Pipe2Args& a) {
    const Chunking c = chunking(a.n);
    if (a.d) hipLaunchKernelGGL((k_pipe2_update<true, true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    else     hipLaunchKernelGGL((k_pipe2_update<false, true>), dim3(c.grid), dim3(kBlock), 0, st, a, c.trips);
    return PRCG_LAUNCH_OK() ? c.grid : -1;
}

}  // namespace prcg
