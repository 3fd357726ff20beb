// gfx950 (MI355X / CDNA4): the one-workgroup solvers of small systems, built from shared parts.
//
// Small systems (n <= 4096): the whole solve in ONE launch of ONE workgroup.  nos7 (n=729) or bcsstk03 (n=112) cannot fill a
// chip; with one launch per kernel they are launch-bound (~12 us per iteration).  Here 1024 threads keep the gather source of
// the product in LDS (double-buffered, like the one-launch schedule of prcg_kernels.hip), the other vectors of their own rows in
// registers, the matrix in registers or LDS, and iterate `iters` times.  Same arithmetic per element as the multi-launch
// kernels (built with -ffp-contract=off); rows are summed left to right from +0.0.  Inner products: thread-sequential over its
// rows (row = tid, tid+1024, ...), wave butterfly, 16 waves in order.  Every thread reaches every barrier (trip counts are
// uniform).
//
// Two methods, each ONE body: small_pipe_pr_body (pipe_pr_cg.py:61-75, with a diagonal scaling :109-193) and small_hs_body
// (hs_cg.py:54-62, :70-131), templated on where the matrix lives (MODE), on the preconditioner (PREC: none, a diagonal scaling, or
// point-block Jacobi with blocks of 1..8 rows -- a batch's only) and on the per-system stop (STOP).
// The single sessions launch them on the launch's SmallArgs (k_small_pipe_pr, k_small_hs; k_small_pipe_pr_stop: a session with a
// residual threshold, the STOP form on the session's own word), a batch on the descriptor of
// workgroup blockIdx.x (k_small_pipe_pr_batch, k_small_hs_batch; with block Jacobi k_small_pipe_pr_blocks, k_small_hs_blocks) -- one body, so that a system of a batch carries the single
// solver's bits.  Host side at the end: the fit rules and the launchers.
#include <hip/hip_runtime.h>

#include "prcg_kernels.h"
#include "prcg_device.hpp"

namespace prcg {
namespace {

static_assert(kPartialStride == 8, "the small-system kernels index the scalar history (PRCG_NUM_SCALARS doubles per iteration) with kPartialStride");
constexpr int kSmallThreads = 1024;
constexpr int kSmallRows = 4;                    // rows per thread -> n <= 4096
constexpr int kSmallMaxN = kSmallThreads * kSmallRows;

// MODE 0: matrix in LDS (any row length, up to 4 rows per thread)
// MODE 1: matrix in REGISTERS: n <= 1024 (one row per thread) and every row <= kSmallRegLen
//         nonzeros -- the paper's small test matrices (nos7: rows of 4-7, bcsstk03: 4-6).
constexpr int kSmallRegLen = 8;
template <int MODE> constexpr int kSmallRowsOf = MODE == 1 ? 1 : kSmallRows;

// ---- the LDS carve-up: two buffers of n V (the gather source and its successor), red[16 waves][K], then (MODE 0) the matrix ----
// V = double2: the pairs (r,s) or (r~,s~) of the pipelined body; V = double: the direction p of Hestenes-Stiefel (red follows on
// an even double).  Each workgroup carves the launch's dynamic LDS by its OWN n and nnz, so a system's bits do not depend on its
// neighbours in the launch.  (small_lds_bytes sizes it for the pairs: more than the directions need.)
template <typename V> struct SmallLds { V* cur; V* nxt; double* red; double* lval; int* lcol; };
template <int MODE, typename V, int K>
__device__ __forceinline__ SmallLds<V> small_carve(int n, int nnz) {
    extern __shared__ __align__(16) unsigned char smem[];
    SmallLds<V> l;
    l.cur = reinterpret_cast<V*>(smem);
    l.nxt = l.cur + n;
    l.red = reinterpret_cast<double*>(l.nxt + n) + (sizeof(V) == sizeof(double) ? (n & 1) : 0);
    l.lval = l.red + 16 * K;
    l.lcol = reinterpret_cast<int*>(l.lval + (MODE == 0 ? nnz : 0));
    return l;
}

// ---- the matrix of a thread's rows ----
template <int MODE> struct SmallMatrix {
    int rbeg[kSmallRowsOf<MODE>], rend[kSmallRowsOf<MODE>];      // row j of the thread: nonzeros [rbeg[j], rend[j])
    const double* lval; const int* lcol;                         // MODE 0: the whole matrix, in LDS
    double rv[kSmallRegLen]; int rc[kSmallRegLen]; int rlen;     // MODE 1: the thread's one row
};
// (the caller's barrier before the first product completes the MODE 0 copy)
template <int MODE>
__device__ __forceinline__ void small_stage(SmallMatrix<MODE>& m, const SmallArgs& a, double* lval, int* lcol) {
    const int tid = threadIdx.x;
#pragma unroll
    for (int j = 0; j < kSmallRowsOf<MODE>; ++j) {
        const int row = tid + j * kSmallThreads;
        m.rbeg[j] = 0; m.rend[j] = 0;
        if (row < a.n) { m.rbeg[j] = a.indptr[row]; m.rend[j] = a.indptr[row + 1]; }
    }
    // MODE 1: this thread's row, padded with (0.0, own column) -- adding +-0.0 products at the
    // END of the row sum cannot change it (x + 0.0 == x, and a finite entry times 0.0 is 0.0;
    // inf/nan entries poison the row either way)... except that 0.0 * inf = nan: so padded
    // slots are skipped by a length test instead of being multiplied.
    if constexpr (MODE == 1) {
        m.rlen = m.rend[0] - m.rbeg[0];
#pragma unroll
        for (int q = 0; q < kSmallRegLen; ++q) {
            const bool ok = q < m.rlen;
            m.rv[q] = ok ? a.val[m.rbeg[0] + q] : 0.0;
            m.rc[q] = ok ? a.col[m.rbeg[0] + q] : 0;
        }
    } else {
        for (int q = tid; q < a.nnz; q += kSmallThreads) { lval[q] = a.val[q]; lcol[q] = a.col[q]; }
        m.lval = lval; m.lcol = lcol;
    }
}
// (A src)_row for row j of the thread, left to right from +0.0; V = double2: both columns of a pair source at once
template <int MODE, typename V>
__device__ __forceinline__ V small_row_product(const SmallMatrix<MODE>& m, int j, const V* src) {
    V sum; vzero(sum);
    if constexpr (MODE == 1) {
        V g[kSmallRegLen];
#pragma unroll
        for (int q = 0; q < kSmallRegLen; ++q) g[q] = src[m.rc[q]];      // all gathers in flight
#pragma unroll
        for (int q = 0; q < kSmallRegLen; ++q)
            if (q < m.rlen) vacc(sum, vmul(m.rv[q], g[q]));
    } else {
        for (int q = m.rbeg[j]; q < m.rend[j]; ++q) vacc(sum, vmul(m.lval[q], src[m.lcol[q]]));
    }
    return sum;
}

// ---- the workgroup's sum of M values per thread, in two halves with the caller's barrier between them ----
// put: wave butterfly, lane 0 of wave w stores red[w][0..M) (rows of K doubles); get: EVERY wave sums the 16 partials of slot q
// with the same butterfly (lanes 0..15 hold them) and broadcasts lane 0's bits.  A second barrier must follow the gets before red
// is put again.
template <int K, int M>
__device__ __forceinline__ void small_red_put(double* red, const double (&acc)[M]) {
    static_assert(M <= K, "red rows hold K doubles");
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double v[M];
#pragma unroll
    for (int q = 0; q < M; ++q) v[q] = wave_sum(acc[q]);
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < M; ++q) red[wv * K + q] = v[q];
    }
}
template <int K>
__device__ __forceinline__ double small_red_get(const double* red, int q) {
    return wave_sum16(red[(threadIdx.x & 15) * K + q]);
}

// ---- point-block Jacobi: the rows of a thread in their blocks ----
// Row start + a of a block of m rows (1..8) forms (M^-1 v)_{start+a} from the block's m entries of v, which its rows exchange
// through LDS, and its own row B[a][0..m) of the block's inverse:  acc = B[a][0] v[start];  acc = acc + B[a][j] v[start+j],
// j = 1 .. m-1 -- every product and sum rounded, the loop of k_block_jacobi_var (prcg_blockjac.hip), so VarBlockJacobi.__call__
// carries its bits.  A block may lie anywhere: across waves, and across rows 1023/1024, ... (a thread's first and second row);
// the barrier between the stores of v and these loads is the caller's.  Where B[a] lives: MODE 1 (one row per thread) in eight
// registers, loaded once per launch; MODE 0 (up to four rows per thread) in memory, read through L2 in every iteration -- 32
// doubles per thread would not fit beside the state, and LDS is the matrix's.  The loads of v are unrolled and predicated like
// the gathers of small_row_product; index min(j, m-1) keeps a load hoisted above its predicate inside the block.
template <int MODE> struct SmallBlockRows {
    int2 tab[kSmallRowsOf<MODE>];                                // row j of the thread: SmallBlocks::tab, {start | m << 16, offset of B[a]}
    const double* inv;                                           // MODE 0: B[a] is read from memory, inv + tab[j].y
    double b[kSmallRegLen];                                      // MODE 1: B[a] of the thread's one row
};
template <int MODE>
__device__ __forceinline__ void small_block_stage(SmallBlockRows<MODE>& k, const SmallBlocks& bk, int n) {
    static_assert(kSmallRegLen == 8, "a block has at most 8 rows");
#pragma unroll
    for (int j = 0; j < kSmallRowsOf<MODE>; ++j) {
        const int row = threadIdx.x + j * kSmallThreads;
        k.tab[j] = make_int2(1 << 16, 0);
        if (row < n) k.tab[j] = bk.tab[row];
    }
    k.inv = bk.inv;
    if constexpr (MODE == 1) {
#pragma unroll
        for (int q = 0; q < 8; ++q) k.b[q] = (threadIdx.x < n && q < (k.tab[0].x >> 16)) ? bk.inv[k.tab[0].y + q] : 0.0;
    }
}
template <int MODE, typename V>
__device__ __forceinline__ V small_block_apply(const SmallBlockRows<MODE>& k, int j, const V* src) {
    const int start = k.tab[j].x & 0xffff, m = k.tab[j].x >> 16;
    if constexpr (MODE == 1) {
        V g[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) g[q] = src[start + (q < m ? q : m - 1)];      // all loads in flight
        V acc = vmul(k.b[0], g[0]);
#pragma unroll
        for (int q = 1; q < 8; ++q)
            if (q < m) vacc(acc, vmul(k.b[q], g[q]));
        return acc;
    } else {
        const double* __restrict__ b = k.inv + k.tab[j].y;
        V acc = vmul(b[0], src[start]);
#pragma unroll 1                                                 // (unrolled, four rows' loads in flight at once spill to scratch)
        for (int q = 1; q < m; ++q) vacc(acc, vmul(b[q], src[start + q]));
        return acc;
    }
}

// ---- stopping a system of a batch at its OWN residual threshold: the STOP form of the bodies (rule: prcg_kernels.h) ----
// Every thread of the workgroup must take the same exit, or some waves would wait at a barrier the others never reach.  The
// operands of the rule are the same bits in all 1024 threads: thr comes from a load of one address that the launch never
// writes; mu, nu, rr are either loaded from one address (row k0 of the scalars, which the launch only reads) or results of
// small_red_get, in which EVERY wave sums the same 16 LDS partials by the same butterfly and broadcasts lane 0's bits -- behind
// the barrier that completes them, which is why every body keeps exactly its barriers.  (The stop word: small_stop_entry.)
// The comparison itself is stop_rule (prcg_device.hpp), shared with the one-launch schedule of single sessions; readfirstlane
// there makes the verdict a scalar, so the branch on it is a scalar branch.
// On entry, before the first barrier: true if this workgroup has nothing to do -- its system stopped in an earlier launch
// (nothing is stored), or the session is at its start and the rule fires on row 0 (thread 0 records {0, status}; the state of
// iteration 0 is already in memory).  b = 0 ends here: rr = 0 <= thr whatever mu is.  No barrier separates thread 0's store from
// a later wave's load of the word: a wave that already sees {0, status} returns by the first test where it would have returned by
// the rule -- the same exit either way.  Every other store to the word follows the body's barriers.
__device__ __forceinline__ bool small_stop_entry(const SmallArgs& a, const SmallStop& st) {
    if (__builtin_amdgcn_readfirstlane(st.word[0]) >= 0) return true;
    if (a.k0 != 0) return false;
    const int v = stop_rule(a.dots[0], a.dots[3], a.dots[4], st.thr);
    if (v && threadIdx.x == 0) { st.word[0] = 0; st.word[1] = v; }
    return v != 0;
}
// after the body's final stores: thread 0 records where and why the system stopped
__device__ __forceinline__ void small_stop_record(const SmallStop& st, int k, int status) {
    if (status && threadIdx.x == 0) { st.word[0] = k; st.word[1] = status; }
}

// ---- pipelined predict-and-recompute (pipe_pr_cg.py:61-75; JAC: with a diagonal scaling d, Jacobi d = 1 / diag A, :109-193) ----
// LDS holds the gather source as pairs, double-buffered: (r,s), with JAC (r~,s~); a thread keeps x, p -- with JAC also r, s and d
// -- of its own rows in registers.  Per row (A r~)_i and (A s~)_i are summed left to right from +0.0, then the expressions and
// order of fused_row_update (prcg_device.hpp) with w = A r~ recomputed.  Without the scaling r~ IS r and s~ IS s: the same
// expressions with d dropped, not multiplied by one.  Sums per iteration: mu = p.s, delta = r.s~, gamma = s~.s, nu = r~.r, with
// JAC also rr = r.r (without: rr = nu): red is [16 waves][4 or 5].  Two barriers per iteration.
// dots[k] = {mu, delta, gamma, nu, rr}, coef[k] = {al, bt, nu_pred}.
// PREC == kSmallPrecBlocks (M^-1 by blocks, bk; jc.ts holds the pairs (r~,s~), jc.d is not read): everything above with u~ and w~
// from the block apply.  The row products of ALL the thread's rows come first and go to LDS as pairs (w,u); one barrier; then
// each row forms (w~,u~) from its block's pairs and goes on as with the scaling.  The pairs go where the successor would
// (nxt), and the successor goes where the source is: once the products are done a row's (r~,s~) in cur is read by its own
// thread only, which overwrites it with the new one -- so the two buffers are not swapped, LDS holds what it holds with the
// scaling, and the iteration has three barriers: cur is gathered from, and nxt written, only behind the two of the sums.
template <int MODE, int PREC, bool STOP>
__device__ __forceinline__ void small_pipe_pr_body(const SmallArgs& a, const SmallJacobi& jc, const SmallBlocks& bk, const SmallStop& stop) {
    if constexpr (STOP) { if (small_stop_entry(a, stop)) return; }
    constexpr bool JAC = PREC != kSmallPrecNone, BLK = PREC == kSmallPrecBlocks;
    constexpr int ROWS = kSmallRowsOf<MODE>, K = JAC ? 5 : 4;
    const int n = a.n, tid = threadIdx.x;
    const SmallLds<double2> l = small_carve<MODE, double2, K>(n, a.nnz);
    const double2* __restrict__ XPg = reinterpret_cast<const double2*>(a.xp);
    const double2* __restrict__ RSg = reinterpret_cast<const double2*>(a.rs);
    const double2* __restrict__ TSg = reinterpret_cast<const double2*>(jc.ts);
    double xr[ROWS], pr[ROWS], rr_[ROWS], sr[ROWS], dr[ROWS];
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const int row = tid + j * kSmallThreads;
        xr[j] = 0.0; pr[j] = 0.0; rr_[j] = 0.0; sr[j] = 0.0; dr[j] = 0.0;
        if (row < n) {
            const double2 xp = XPg[row];
            const double2 rs = RSg[row];
            xr[j] = xp.x; pr[j] = xp.y;
            if constexpr (JAC) { rr_[j] = rs.x; sr[j] = rs.y; l.cur[row] = TSg[row]; }
            else l.cur[row] = rs;
            if constexpr (PREC == kSmallPrecJacobi) dr[j] = jc.d[row];
        }
    }
    SmallMatrix<MODE> m;
    small_stage<MODE>(m, a, l.lval, l.lcol);
    SmallBlockRows<MODE> kb;
    if constexpr (BLK) small_block_stage<MODE>(kb, bk, n);
    // inner products of the incoming state
    const double* row0 = a.dots + (size_t)a.k0 * kPartialStride;
    double mu = row0[0], dl = row0[1], gm = row0[2], nu = row0[3];
    __syncthreads();

    double2* cur = l.cur;
    double2* nxt = l.nxt;
    int stop_k = 0, stop_status = 0;                             // STOP: where and why the loop was left early
    const double stop_thr = stop.thr;                            // (read once: the loop's stores could alias the descriptor)
    for (int it = 1; it <= a.iters; ++it) {
        // coefficients (pipe_pr_cg.py:64-66,75; :174-175,187), identical in every thread
        const double al = nu / mu;
        const double a2 = al * al;
        const double nup = a.meurant ? (-nu + a2 * gm) : ((nu - (2 * al) * dl) + a2 * gm);
        const double bt = nup / nu;
        if (tid == 0) {
            double* cf = a.coef + (size_t)(a.k0 + it) * 4;
            cf[0] = al; cf[1] = bt; cf[2] = nup;
        }
        double acc[K] = {};
        double2 wu1;                                             // MODE 1 keeps its row's pair; MODE 0 reads its rows' back
        if constexpr (BLK) {                                     // every row's (w,u) to its block's rows
#pragma unroll
            for (int j = 0; j < ROWS; ++j) {
                const int row = tid + j * kSmallThreads;
                if (row < n) { wu1 = small_row_product<MODE>(m, j, cur); nxt[row] = wu1; }
            }
            lds_barrier();                                       // the pairs are complete, and cur has been gathered from
        }
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const int row = tid + j * kSmallThreads;
            if (row < n) {
                double2 wu;                                      // w = (A r~)_i, u = (A s~)_i
                if constexpr (BLK) wu = MODE == 1 ? wu1 : nxt[row];
                else wu = small_row_product<MODE>(m, j, cur);
                const double2 ts = cur[row];
                xr[j] = xr[j] + al * pr[j];                      // x += a p
                const double rtn = ts.x - al * ts.y;             // r~ -= a s~
                const double wn = wu.x - al * wu.y;              // w -= a u
                double rn = rtn, sn, stn;
                if constexpr (JAC) {
                    double ut, wt;
                    if constexpr (BLK) {
                        const double2 t = small_block_apply<MODE>(kb, j, nxt);
                        wt = t.x; ut = t.y;                      // w~ = M^-1 w, u~ = M^-1 u
                    } else {
                        ut = dr[j] * wu.y;                       // u~ = M^-1 u
                        wt = dr[j] * wu.x;                       // w~ = M^-1 w
                    }
                    rn = rr_[j] - al * sr[j];                    // r -= a s
                    const double wtn = wt - al * ut;             // w~ -= a u~
                    sn = wn + bt * sr[j];                        // s = w + b s
                    stn = wtn + bt * ts.y;                       // s~ = w~ + b s~
                    rr_[j] = rn; sr[j] = sn;
                } else {
                    sn = wn + bt * ts.y;                         // s = w + b s
                    stn = sn;
                }
                const double pn = rtn + bt * pr[j];              // p = r~ + b p
                pr[j] = pn;
                if constexpr (BLK) cur[row] = make_double2(rtn, stn);
                else nxt[row] = make_double2(rtn, stn);
                acc[0] += pn * sn; acc[1] += rn * stn; acc[2] += stn * sn; acc[3] += rtn * rn;
                if constexpr (JAC) acc[4] += rn * rn;
            }
        }
        small_red_put<K>(l.red, acc);
        lds_barrier();                                           // nxt complete, red complete
        mu = small_red_get<K>(l.red, 0);
        dl = small_red_get<K>(l.red, 1);
        gm = small_red_get<K>(l.red, 2);
        nu = small_red_get<K>(l.red, 3);
        double rr = nu;
        if constexpr (JAC) rr = small_red_get<K>(l.red, 4);
        if (tid == 0) {
            double* d = a.dots + (size_t)(a.k0 + it) * kPartialStride;
            d[0] = mu; d[1] = dl; d[2] = gm; d[3] = nu; d[4] = rr;
        }
        lds_barrier();                                           // everybody has read red before it is rewritten
        if constexpr (!BLK) { double2* tmp = cur; cur = nxt; nxt = tmp; }
        if constexpr (STOP) {                                    // the iteration is complete: the rule, on this iterate's scalars
            stop_status = stop_rule(mu, nu, rr, stop_thr);
            if (stop_status) { stop_k = a.k0 + it; break; }
        }
    }

    double2* XPo = reinterpret_cast<double2*>(a.xp);
    double2* RSo = reinterpret_cast<double2*>(a.rs);
    double2* TSo = reinterpret_cast<double2*>(jc.ts);
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const int row = tid + j * kSmallThreads;
        if (row < n) {
            XPo[row] = make_double2(xr[j], pr[j]);
            if constexpr (JAC) { RSo[row] = make_double2(rr_[j], sr[j]); TSo[row] = cur[row]; }
            else RSo[row] = cur[row];
        }
    }
    if constexpr (STOP) small_stop_record(stop, stop_k, stop_status);
}

// ---- Hestenes-Stiefel (hs_cg.py:54-62; JAC: with the same scaling, :70-131) ----
// BASELINE config 1 is bcsstk03 (n = 112) under hs_cg: two launches and two kernel boundaries per iteration cost it 9-10 us each.
// The storage of the pipelined body (matrix in registers or LDS, the gather source in LDS: here the direction p, double-buffered);
// x, r, p, s (and d) of a thread's rows live in its registers.  Per iteration, with the expressions and roundings of
// k_hs_update_xr / k_hs_update_p / the row sums of csr_matvec:  a = nu / mu;  x += a p;  r -= a s;  [r~ = d r, formed in
// registers;]  nu' = r.r~ [and rr = r.r, the same sum without the scaling];  b = nu' / nu;  p = r~ + b p;  s = A p;  mu = p.s  --
// two reduction points (the two reductions that make Hestenes-Stiefel what it is), four barriers; red is [16 waves][1 or 2].
// Scalars as the launches leave them: dots[k] = {mu_k, -, -, nu_k, rr_k}, coef[k] = {a_k, b_k}.
// PREC == kSmallPrecBlocks: r~ = M^-1 r by blocks (bk).  The new r of every row goes to `nxt` -- free until the new direction
// is stored there, behind the barrier of nu' --, one barrier, then each row forms r~ from its block's entries: five barriers.
template <int MODE, int PREC, bool STOP>
__device__ __forceinline__ void small_hs_body(const SmallArgs& a, const SmallJacobi& jc, const SmallBlocks& bk, const SmallStop& stop) {
    if constexpr (STOP) { if (small_stop_entry(a, stop)) return; }
    constexpr bool JAC = PREC != kSmallPrecNone, BLK = PREC == kSmallPrecBlocks;
    constexpr int ROWS = kSmallRowsOf<MODE>, K = JAC ? 2 : 1;
    const int n = a.n, tid = threadIdx.x;
    const SmallLds<double> l = small_carve<MODE, double, K>(n, a.nnz);
    double xr[ROWS], rr_[ROWS], pr[ROWS], sr[ROWS], dr[ROWS];
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const int row = tid + j * kSmallThreads;
        xr[j] = 0.0; rr_[j] = 0.0; pr[j] = 0.0; sr[j] = 0.0; dr[j] = 0.0;
        if (row < n) {
            xr[j] = a.xp[row]; rr_[j] = a.rs[row]; pr[j] = a.hs_p[row]; sr[j] = a.hs_s[row];
            if constexpr (PREC == kSmallPrecJacobi) dr[j] = jc.d[row];
            l.cur[row] = pr[j];
        }
    }
    SmallMatrix<MODE> m;
    small_stage<MODE>(m, a, l.lval, l.lcol);
    SmallBlockRows<MODE> kb;
    if constexpr (BLK) small_block_stage<MODE>(kb, bk, n);
    double mu = a.dots[(size_t)a.k0 * kPartialStride + 0], nu = a.dots[(size_t)a.k0 * kPartialStride + 3];
    __syncthreads();

    double* cur = l.cur;                                         // holds p_{k-1}
    double* nxt = l.nxt;
    int stop_k = 0, stop_status = 0;                             // STOP: where and why the loop was left early
    const double stop_thr = stop.thr;                            // (read once: the loop's stores could alias the descriptor)
    for (int it = 1; it <= a.iters; ++it) {
        const double al = nu / mu;                               // a = nu / mu                       hs_cg.py:55, :116
        double rt[ROWS];                                         // r~ (without the scaling: r)
        double acc[K] = {};
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            rt[j] = 0.0;
            if (tid + j * kSmallThreads < n) {
                xr[j] = xr[j] + al * pr[j];                      // x += a p
                rr_[j] = rr_[j] - al * sr[j];                    // r -= a s
                if constexpr (BLK) {
                    nxt[tid + j * kSmallThreads] = rr_[j];       // ... to its block's rows
                } else {
                    rt[j] = rr_[j];
                    if constexpr (JAC) rt[j] = dr[j] * rr_[j];   // r~ = M^-1 r                        :118
                    acc[0] += rr_[j] * rt[j];
                    if constexpr (JAC) acc[1] += rr_[j] * rr_[j];
                }
            }
        }
        if constexpr (BLK) {
            lds_barrier();                                       // r complete
#pragma unroll
            for (int j = 0; j < ROWS; ++j) {
                if (tid + j * kSmallThreads < n) {
                    rt[j] = small_block_apply<MODE>(kb, j, nxt); // r~ = M^-1 r
                    acc[0] += rr_[j] * rt[j];
                    acc[1] += rr_[j] * rr_[j];
                }
            }
        }
        small_red_put<K>(l.red, acc);
        lds_barrier();
        const double nun = small_red_get<K>(l.red, 0);           // nu' = r.r~                         :58, :119
        double rrn = nun;
        if constexpr (JAC) rrn = small_red_get<K>(l.red, 1);     // rr = r.r
        const double bt = nun / nu;                              // b = nu' / nu                       :59
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            const int row = tid + j * kSmallThreads;
            if (row < n) { pr[j] = rt[j] + bt * pr[j]; nxt[row] = pr[j]; }      // p = r~ + b p          :60
        }
        lds_barrier();                                           // the new direction is complete (and red has been read)
        double accm[1] = {0.0};
#pragma unroll
        for (int j = 0; j < ROWS; ++j) {
            if (tid + j * kSmallThreads < n) {
                sr[j] = small_row_product<MODE>(m, j, nxt);      // s = A p                            :61
                accm[0] += pr[j] * sr[j];
            }
        }
        small_red_put<K>(l.red, accm);
        lds_barrier();
        mu = small_red_get<K>(l.red, 0);                         // mu = p.s                           :62
        if (tid == 0) {
            double* cf = a.coef + (size_t)(a.k0 + it) * 4;
            cf[0] = al; cf[1] = bt;
            double* d = a.dots + (size_t)(a.k0 + it) * kPartialStride;
            d[0] = mu; d[3] = nun; d[4] = rrn;
        }
        nu = nun;
        lds_barrier();                                           // everybody has read red before it is rewritten
        double* tmp = cur; cur = nxt; nxt = tmp;
        if constexpr (STOP) {                                    // the iteration is complete: the rule, on this iterate's scalars
            stop_status = stop_rule(mu, nu, rrn, stop_thr);
            if (stop_status) { stop_k = a.k0 + it; break; }
        }
    }
#pragma unroll
    for (int j = 0; j < ROWS; ++j) {
        const int row = tid + j * kSmallThreads;
        if (row < n) { a.xp[row] = xr[j]; a.rs[row] = rr_[j]; a.hs_p[row] = pr[j]; a.hs_s[row] = sr[j]; }
    }
    if constexpr (STOP) small_stop_record(stop, stop_k, stop_status);
}

// ---- the single sessions: one workgroup, the launch's SmallArgs ----
template <int MODE>
__global__ __launch_bounds__(kSmallThreads) void k_small_pipe_pr(SmallArgs a) { small_pipe_pr_body<MODE, kSmallPrecNone, false>(a, SmallJacobi{}, SmallBlocks{}, SmallStop{}); }
template <int MODE>
__global__ __launch_bounds__(kSmallThreads) void k_small_hs(SmallArgs a) { small_hs_body<MODE, kSmallPrecNone, false>(a, SmallJacobi{}, SmallBlocks{}, SmallStop{}); }
// ... stopped at a residual threshold (prcg_set_stop): the STOP form of the body on the session's own word
template <int MODE>
__global__ __launch_bounds__(kSmallThreads) void k_small_pipe_pr_stop(SmallArgs a, SmallStop stop) { small_pipe_pr_body<MODE, kSmallPrecNone, true>(a, SmallJacobi{}, SmallBlocks{}, stop); }
// ... and the Hestenes-Stiefel single session (prcg_set_stop_hs): what a system of a batch with a threshold runs, on the session's word
template <int MODE>
__global__ __launch_bounds__(kSmallThreads) void k_small_hs_stop(SmallArgs a, SmallStop stop) { small_hs_body<MODE, kSmallPrecNone, true>(a, SmallJacobi{}, SmallBlocks{}, stop); }

// ---- a BATCH of small systems: one launch, workgroup blockIdx.x solves system desc[blockIdx.x] (prcg_batch.cpp) ----
// The descriptors live in device memory, one SmallArgs per system with pointers into the batch's concatenated matrix, state,
// scalar and coefficient buffers; blockIdx.x is uniform, so a workgroup reads its descriptor with uniform loads.  Where the
// session stands (k0, iters, meurant) is the same for every system and comes with the launch.  jac[blockIdx.x] and
// stop[blockIdx.x] belong to desc[blockIdx.x]; they are read by the JAC / STOP instantiations only.
struct SmallSystem { SmallArgs a; SmallJacobi jac; SmallStop stop; };
template <bool JAC, bool STOP>
__device__ __forceinline__ SmallSystem small_system(const SmallBatchArgs& g) {
    SmallSystem s{g.desc[blockIdx.x], SmallJacobi{}, SmallStop{}};
    s.a.k0 = g.k0; s.a.iters = g.iters; s.a.meurant = g.meurant;
    if constexpr (JAC) s.jac = g.jac[blockIdx.x];
    if constexpr (STOP) s.stop = g.stop[blockIdx.x];
    return s;
}
template <int MODE, bool JAC, bool STOP>
__global__ __launch_bounds__(kSmallThreads) void k_small_pipe_pr_batch(SmallBatchArgs g) {
    const SmallSystem s = small_system<JAC, STOP>(g);
    small_pipe_pr_body<MODE, JAC ? kSmallPrecJacobi : kSmallPrecNone, STOP>(s.a, s.jac, SmallBlocks{}, s.stop);
}
template <int MODE, bool JAC, bool STOP>
__global__ __launch_bounds__(kSmallThreads) void k_small_hs_batch(SmallBatchArgs g) {
    const SmallSystem s = small_system<JAC, STOP>(g);
    small_hs_body<MODE, JAC ? kSmallPrecJacobi : kSmallPrecNone, STOP>(s.a, s.jac, SmallBlocks{}, s.stop);
}
// ... preconditioned by point-block Jacobi: blk[blockIdx.x] belongs to desc[blockIdx.x] (g.jac is not read)
template <int MODE, bool STOP>
__global__ __launch_bounds__(kSmallThreads) void k_small_pipe_pr_blocks(SmallBatchArgs g, const SmallBlocks* __restrict__ blk) {
    const SmallSystem s = small_system<false, STOP>(g);
    const SmallBlocks bk = blk[blockIdx.x];
    small_pipe_pr_body<MODE, kSmallPrecBlocks, STOP>(s.a, SmallJacobi{bk.ts, nullptr}, bk, s.stop);
}
template <int MODE, bool STOP>
__global__ __launch_bounds__(kSmallThreads) void k_small_hs_blocks(SmallBatchArgs g, const SmallBlocks* __restrict__ blk) {
    const SmallSystem s = small_system<false, STOP>(g);
    small_hs_body<MODE, kSmallPrecBlocks, STOP>(s.a, SmallJacobi{}, blk[blockIdx.x], s.stop);
}

// Initial state of every system of a batch in ONE launch (pipe_pr_cg.py:22-28, :122-140; hs_cg.py:22-27, :84-90), workgroup
// blockIdx.x for system desc[blockIdx.x]:  x = x0;  r = b - A x0;  [r~ = d r;]  p = r~;  s = A p;  [pipelined: s~ = d s]  -- row
// sums left to right from +0.0 and the expressions of the single session's start-up launches, so the vectors carry its bits --
// and the inner products of row 0 of the scalars (pipelined {p.s, r.s~, s~.s, r~.r, r.r}, Hestenes-Stiefel {p.s, -, -, r~.r, r.r};
// without the scaling r~ IS r, s~ IS s), summed in the order of the LOOP: thread-sequential over rows tid, tid + 1024, ..., wave
// butterfly, 16 waves.  (The single session sums its initial products in the order of its start-up launches: row 0 may differ
// from it in the last bit.)  The matrix is read from memory: once.
// PREC == kSmallPrecBlocks: r~ = M^-1 r and s~ = M^-1 s by blocks (blk[blockIdx.x]; small_block_apply, the blocks' rows read from
// memory).  The rows of a block exchange r, then s, through pl, each time between two barriers.
template <bool HS, int PREC>
__global__ __launch_bounds__(kSmallThreads) void k_small_batch_init(const SmallArgs* __restrict__ desc, const SmallInit* __restrict__ init,
                                                                    const SmallJacobi* __restrict__ jac, const SmallBlocks* __restrict__ blk) {
    constexpr bool JAC = PREC != kSmallPrecNone, BLK = PREC == kSmallPrecBlocks;
    constexpr int K = JAC ? 5 : 4;
    __shared__ double pl[kSmallMaxN];                            // p (= r~): the source of s = A p
    __shared__ double red[16 * K];
    const SmallArgs a = desc[blockIdx.x];
    const SmallInit in = init[blockIdx.x];
    SmallJacobi jc{};
    if constexpr (PREC == kSmallPrecJacobi) jc = jac[blockIdx.x];
    const int n = a.n, tid = threadIdx.x;
    SmallBlockRows<0> kb;
    if constexpr (BLK) { const SmallBlocks bk = blk[blockIdx.x]; jc.ts = bk.ts; small_block_stage<0>(kb, bk, n); }
    double xr[kSmallRows], rr_[kSmallRows], rt[kSmallRows];
#pragma unroll
    for (int j = 0; j < kSmallRows; ++j) {
        const int row = tid + j * kSmallThreads;
        xr[j] = 0.0; rr_[j] = 0.0; rt[j] = 0.0;
        if (row < n) {
            double t = 0.0;                                      // (A x0)_i, left to right
            for (int q = a.indptr[row]; q < a.indptr[row + 1]; ++q) t += a.val[q] * in.x0[a.col[q]];
            xr[j] = in.x0[row];                                  // x = x0
            rr_[j] = in.b[row] - t;                              // r = b - A x
            rt[j] = rr_[j];
            if constexpr (PREC == kSmallPrecJacobi) rt[j] = jc.d[row] * rr_[j];       // r~ = M^-1 r
            pl[row] = rt[j];
        }
    }
    __syncthreads();
    if constexpr (BLK) {                                         // pl holds r: r~ = M^-1 r, then pl holds p = r~
#pragma unroll
        for (int j = 0; j < kSmallRows; ++j)
            if (tid + j * kSmallThreads < n) rt[j] = small_block_apply<0>(kb, j, pl);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kSmallRows; ++j)
            if (tid + j * kSmallThreads < n) pl[tid + j * kSmallThreads] = rt[j];
        __syncthreads();
    }
    double spv[BLK ? kSmallRows : 1];
    if constexpr (BLK && !HS) {                                  // s = A p of every row, exchanged through pl for s~ = M^-1 s
#pragma unroll
        for (int j = 0; j < kSmallRows; ++j) {
            const int row = tid + j * kSmallThreads;
            spv[j] = 0.0;
            if (row < n)
                for (int q = a.indptr[row]; q < a.indptr[row + 1]; ++q) spv[j] += a.val[q] * pl[a.col[q]];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kSmallRows; ++j)
            if (tid + j * kSmallThreads < n) pl[tid + j * kSmallThreads] = spv[j];
        __syncthreads();
    }
    double acc[K] = {};
#pragma unroll
    for (int j = 0; j < kSmallRows; ++j) {
        const int row = tid + j * kSmallThreads;
        if (row < n) {
            double sp = 0.0;                                     // (A p)_i, p = r~, left to right
            if constexpr (BLK && !HS) sp = spv[j];
            else
                for (int q = a.indptr[row]; q < a.indptr[row + 1]; ++q) sp += a.val[q] * pl[a.col[q]];
            const double rn = rr_[j], pn = rt[j];
            if constexpr (HS) {
                a.xp[row] = xr[j]; a.rs[row] = rn; a.hs_p[row] = pn; a.hs_s[row] = sp;
            } else {
                double stn = sp;
                if constexpr (PREC == kSmallPrecJacobi) stn = jc.d[row] * sp;         // s~ = M^-1 s
                if constexpr (BLK) stn = small_block_apply<0>(kb, j, pl);
                reinterpret_cast<double2*>(a.xp)[row] = make_double2(xr[j], pn);
                reinterpret_cast<double2*>(a.rs)[row] = make_double2(rn, sp);
                if constexpr (JAC) reinterpret_cast<double2*>(jc.ts)[row] = make_double2(pn, stn);
                acc[1] += rn * stn; acc[2] += stn * sp;          // r.s~, s~.s
            }
            acc[0] += pn * sp; acc[3] += pn * rn;                // p.s, r~.r
            if constexpr (JAC) acc[4] += rn * rn;                // r.r
        }
    }
    small_red_put<K>(red, acc);
    __syncthreads();
    const double mu = small_red_get<K>(red, 0), dl = small_red_get<K>(red, 1), gm = small_red_get<K>(red, 2), nu = small_red_get<K>(red, 3);
    double rr = nu;
    if constexpr (JAC) rr = small_red_get<K>(red, 4);
    if (tid == 0) {
        double* d = a.dots;                                      // row 0
        d[0] = mu; d[3] = nu; d[4] = rr;
        if constexpr (!HS) { d[1] = dl; d[2] = gm; }
    }
}

}  // namespace

// ---- host side: the fit rules ----
size_t small_lds_bytes(int n, int nnz, int mode, int prec) {
    return (size_t)2 * n * 16 + (prec ? 80 : 64) * 8 + (mode == 0 ? (size_t)nnz * 12 + 16 : 0);
}
// mode 1 (matrix in registers) if n <= 1024 and the longest row has <= 8 nonzeros; mode 0
// (matrix in LDS) if it fits beside the vectors; otherwise the multi-launch schedule is
// faster (measured: bcsstk14, 63 k nonzeros re-read through L2 by one CU: 58 us/iteration).
constexpr size_t kSmallLdsCap = 156 * 1024;
bool small_fits(int64_t n, int64_t nnz, int max_row_len, int* mode, int prec) {
    if (n < 1 || n > kSmallMaxN) return false;
    if (n <= kSmallThreads && max_row_len <= kSmallRegLen) { *mode = 1; return true; }
    if (nnz < (1 << 20) && small_lds_bytes((int)n, (int)nnz, 0, prec) <= kSmallLdsCap && max_row_len <= 64) { *mode = 0; return true; }
    return false;
}

// ---- host side: the launchers ----
namespace {
using SmallBatchFn = void (*)(SmallBatchArgs);
using SmallSingleFn = void (*)(SmallArgs);
// [hs][mode][jacobi][stop]
const SmallBatchFn kSmallBatchFn[2][2][2][2] = {
    {{{k_small_pipe_pr_batch<0, false, false>, k_small_pipe_pr_batch<0, false, true>},
      {k_small_pipe_pr_batch<0, true, false>, k_small_pipe_pr_batch<0, true, true>}},
     {{k_small_pipe_pr_batch<1, false, false>, k_small_pipe_pr_batch<1, false, true>},
      {k_small_pipe_pr_batch<1, true, false>, k_small_pipe_pr_batch<1, true, true>}}},
    {{{k_small_hs_batch<0, false, false>, k_small_hs_batch<0, false, true>}, {k_small_hs_batch<0, true, false>, k_small_hs_batch<0, true, true>}},
     {{k_small_hs_batch<1, false, false>, k_small_hs_batch<1, false, true>}, {k_small_hs_batch<1, true, false>, k_small_hs_batch<1, true, true>}}}};
using SmallBlocksFn = void (*)(SmallBatchArgs, const SmallBlocks*);
// [hs][mode][stop]
const SmallBlocksFn kSmallBlocksFn[2][2][2] = {
    {{k_small_pipe_pr_blocks<0, false>, k_small_pipe_pr_blocks<0, true>}, {k_small_pipe_pr_blocks<1, false>, k_small_pipe_pr_blocks<1, true>}},
    {{k_small_hs_blocks<0, false>, k_small_hs_blocks<0, true>}, {k_small_hs_blocks<1, false>, k_small_hs_blocks<1, true>}}};
const SmallSingleFn kSmallSingleFn[2][2] = {{k_small_pipe_pr<0>, k_small_pipe_pr<1>}, {k_small_hs<0>, k_small_hs<1>}};      // [hs][mode]
using SmallSingleStopFn = void (*)(SmallArgs, SmallStop);
const SmallSingleStopFn kSmallSingleStopFn[2][2] = {{k_small_pipe_pr_stop<0>, k_small_pipe_pr_stop<1>}, {k_small_hs_stop<0>, k_small_hs_stop<1>}};      // [hs][mode]

// The kernels may ask for more dynamic LDS than the default 64 KB.  The attribute belongs to the CURRENT device: set for all of
// them on first use on each device, and only a SUCCESSFUL round counts as done.
bool small_lds_attribute() {
    constexpr int kMaxDev = 64;
    static bool attr_done[kMaxDev] = {};
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return false;
    if (dev < kMaxDev && attr_done[dev]) return true;
    const auto set = [](const void* f) { return hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess; };
    for (int i = 0; i < 16; ++i)
        if (!set(reinterpret_cast<const void*>((&kSmallBatchFn[0][0][0][0])[i]))) return false;
    for (int i = 0; i < 8; ++i)
        if (!set(reinterpret_cast<const void*>((&kSmallBlocksFn[0][0][0])[i]))) return false;
    for (int i = 0; i < 4; ++i)
        if (!set(reinterpret_cast<const void*>((&kSmallSingleFn[0][0])[i]))) return false;
    for (int i = 0; i < 4; ++i)
        if (!set(reinterpret_cast<const void*>((&kSmallSingleStopFn[0][0])[i]))) return false;
    if (dev < kMaxDev) attr_done[dev] = true;
    return true;
}
int launch_small_single(hipStream_t st, const SmallArgs& a, int mode, bool hs, const SmallStop* stop) {
    if (!small_lds_attribute()) return -1;
    if (stop) hipLaunchKernelGGL(kSmallSingleStopFn[hs][mode == 1], dim3(1), dim3(kSmallThreads), small_lds_bytes(a.n, a.nnz, mode), st, a, *stop);
    else hipLaunchKernelGGL(kSmallSingleFn[hs][mode == 1], dim3(1), dim3(kSmallThreads), small_lds_bytes(a.n, a.nnz, mode), st, a);
    return hipGetLastError() == hipSuccess ? 1 : -1;
}
}  // namespace

int launch_small_pipe_pr(hipStream_t st, const SmallArgs& a, int mode, const SmallStop* stop) { return launch_small_single(st, a, mode, false, stop); }
// (xp = x, rs = r, hs_p = p, hs_s = s: separate arrays, as the Hestenes-Stiefel sessions hold them)
int launch_small_hs(hipStream_t st, const SmallArgs& a, int mode, const SmallStop* stop) { return launch_small_single(st, a, mode, true, stop); }

// ---- batch of small systems: `count` workgroups, one per descriptor (all of one mode; lds: the largest small_lds_bytes among them)
int launch_small_batch_init(hipStream_t st, const SmallArgs* desc, const SmallInit* init, const SmallJacobi* jac, int count, bool hs,
                            const SmallBlocks* blk) {
    const int prec = blk ? kSmallPrecBlocks : jac ? kSmallPrecJacobi : kSmallPrecNone;
    decltype(&k_small_batch_init<false, 0>) const fn[2][3] = {
        {k_small_batch_init<false, kSmallPrecNone>, k_small_batch_init<false, kSmallPrecJacobi>, k_small_batch_init<false, kSmallPrecBlocks>},
        {k_small_batch_init<true, kSmallPrecNone>, k_small_batch_init<true, kSmallPrecJacobi>, k_small_batch_init<true, kSmallPrecBlocks>}};
    hipLaunchKernelGGL(fn[hs][prec], dim3(count), dim3(kSmallThreads), 0, st, desc, init, jac, blk);
    return hipGetLastError() == hipSuccess ? count : -1;
}
int launch_small_batch(hipStream_t st, const SmallBatchArgs& g, int count, int mode, size_t lds, bool hs, const SmallBlocks* blk) {
    if (!small_lds_attribute()) return -1;
    if (blk) hipLaunchKernelGGL(kSmallBlocksFn[hs][mode == 1][g.stop != nullptr], dim3(count), dim3(kSmallThreads), lds, st, g, blk);
    else hipLaunchKernelGGL(kSmallBatchFn[hs][mode == 1][g.jac != nullptr][g.stop != nullptr], dim3(count), dim3(kSmallThreads), lds, st, g);
    return hipGetLastError() == hipSuccess ? count : -1;
}

}  // namespace prcg
