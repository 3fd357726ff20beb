// libprcg.so engine: handle, operator upload (planned in prcg_plan.cpp), solver sessions, multi-GPU schedule.
// Implements include/prcg.h.  Host code only; kernels live in prcg_kernels.hip.
//
// Per-iteration schedule of the pipelined variants (the GPU form of the PETSc plug-in's
// VecDotBegin / PetscCommSplitReductionBegin / KSP_MatMult / VecDotEnd sequence,
// scaling_experiments_petsc/cg_impls/pipeprcg.c:154-173):
//
//   compute stream : [update k: x,r,p,s + dot partials] -E1-> [SpMM interior rows]
//                    -wait Eh-> [SpMM rows touching ghosts] -wait Er-> [update k+1]
//   comm stream    : wait E1 -> [pack halo] [ncclSend/Recv] -Eh-> [reduce partials]
//                    [ncclAllReduce, 5 doubles] -Er->
//
// i.e. ONE reduction per iteration, hidden behind the matrix product.  The host only
// enqueues; it never synchronises inside prcg_iterate.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <new>
#include <utility>
#include <string>
#include <array>
#include <vector>

#include "../../include/prcg.h"
#include "../../include/prcg_test.h"
#include "prcg_kernels.h"
#include "prcg_batch.h"
#include "prcg_bjvar.h"
#include "prcg_plan.h"
#include "prcg_rccl.h"

using namespace prcg;

namespace {

std::string g_last_error;   // errors with no handle to hang them on

constexpr int kNS = PRCG_NUM_SCALARS;
static_assert(kPartialStride == PRCG_NUM_SCALARS, "the small-system kernel indexes the scalar history with kPartialStride");
constexpr int kCoefStride = 4;
static_assert(kCoefStride == kPr2CoefStride, "k_pr2_update steps from column 0's coefficient row to column 1's");
constexpr int kMaxProfSamples = 512;

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;      // size asked for
    size_t cap = 0;        // size of the allocation
    ~DevBuf() { release(); }
    void release() { if (p) { (void)hipFree(p); p = nullptr; bytes = 0; cap = 0; } }
    hipError_t alloc(size_t nbytes, bool zero = true) {
        release();
        if (nbytes == 0) nbytes = 16;
        hipError_t e = hipMalloc(&p, nbytes);
        if (e != hipSuccess) { p = nullptr; return e; }
        bytes = cap = nbytes;
        if (zero) {
            // the null stream does not order with our non-blocking streams: wait here
            e = hipMemset(p, 0, nbytes);
            if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
        }
        return e;
    }
    // Session state: keep the allocation of the previous solve when it is large enough (a sweep of
    // solves on one operator -- figure_gen.py:343-363 runs nine variants per matrix -- then allocates
    // once) and clear it on the stream the session works on: no hipMalloc, no host synchronisation.
    hipError_t ensure(size_t nbytes, hipStream_t st) {
        if (nbytes == 0) nbytes = 16;
        if (!p || cap < nbytes || cap > 2 * nbytes + (1u << 20)) {
            release();
            hipError_t e = hipMalloc(&p, nbytes);
            if (e != hipSuccess) { p = nullptr; return e; }
            cap = nbytes;
        }
        bytes = nbytes;
        return hipMemsetAsync(p, 0, nbytes, st);
    }
    double* d() const { return static_cast<double*>(p); }
    int* i() const { return static_cast<int*>(p); }
};

struct EventPair { hipEvent_t a = nullptr, b = nullptr; };

// The resident operator: what plan_operator decided (OperatorShape) and the arrays prcg_set_csr uploaded.
struct Operator : OperatorShape {
    bool have_csr = false;
    DevBuf indptr, col, val, tiles;
    DevBuf col16, col8, tile_base;       // 16- / 8-bit tile-relative column encodings (see CsrDev)
    DevBuf vidx8, vdict, vdesc;          // value dictionary (see CsrDev): 1-byte indices, entries, {first,count} per tile
    DevBuf wpat, wtiles, wcw, wvidx, wvdict, wrel;      // window tiles (prcg_win.hip)
    DevBuf sval, scol, sslices, srows, sgran;            // sliced rows (prcg_sell.hip)

    // operator view for a launch over tiles [first, ...): interior launches pass first = 0,
    // boundary launches first = nt_int; a launch over ALL tiles needs both classes to qualify
    CsrDev csr(int first = 0, bool all = true) const {
        const bool boundary = first >= nt_int && nt_bnd > 0;
        const bool ok = all ? (c16_int && (nt_bnd == 0 || c16_bnd)) : (boundary ? c16_bnd : c16_int);
        const bool ok8 = all ? (c8_int && (nt_bnd == 0 || c8_bnd)) : (boundary ? c8_bnd : c8_int);
        const bool okv = all ? (vd_int && (nt_bnd == 0 || vd_bnd)) : (boundary ? vd_bnd : vd_int);
        return CsrDev{indptr.i(), col.i(), val.d(), ok ? static_cast<const unsigned short*>(col16.p) : nullptr,
                      ok8 ? static_cast<const unsigned char*>(col8.p) : nullptr,
                      (ok || ok8) ? static_cast<const int*>(tile_base.p) + first : nullptr,
                      okv ? static_cast<const unsigned char*>(vidx8.p) : nullptr,
                      okv ? static_cast<const double*>(vdict.p) : nullptr,
                      okv ? static_cast<const int2*>(vdesc.p) + first : nullptr};
    }
    const Tile* tile_ptr(int first = 0) const { return static_cast<const Tile*>(tiles.p) + first; }
    WinDev wdev(bool big_ok) const {
        const bool b16 = win_geom >= 2;
        return WinDev{indptr.i(), val.d(), b16 ? nullptr : static_cast<const unsigned char*>(wcw.p),
                      b16 ? static_cast<const unsigned short*>(wcw.p) : nullptr,
                      win_vd ? static_cast<const unsigned char*>(wvidx.p) : nullptr,
                      win_vd ? static_cast<const double*>(wvdict.p) : nullptr,
                      static_cast<const unsigned short*>(wrel.p), static_cast<const PatRec*>(wpat.p), sweep_waves, sweep_tiles, big_ok ? 1 : 0,
                      win_period};
    }
    const WTile* wtile_ptr(int first = 0) const { return static_cast<const WTile*>(wtiles.p) + first; }
    SellDev sdev() const { return SellDev{indptr.i(), val_sell(), static_cast<const unsigned short*>(scol.p), static_cast<const int*>(srows.p), sell_nt, sell_run, sell_window > 0 ? static_cast<const int*>(sgran.p) : nullptr, sell_window}; }
    const double* val_sell() const { return static_cast<const double*>(sval.p); }
    const void* sslice_ptr(int first = 0) const { return static_cast<const char*>(sslices.p) + (size_t)first * 32; }
};

// Everything that describes the OPEN session and nothing that outlives it.  open_session assigns Session{} -- the only
// such assignment -- so a session inherits no flag, pointer or pending state from the one before.
//
// Resets that are NEW against the engine before Session existed (there each family of prcg_solve_begin cleared only what
// it used), and who read the stale value:
//   fused_comm, peer     after a communicator session with PRCG_FUSED_COMM=1 / peer exchange, in every later non-pipelined
//                        or two-RHS session: prcg_schedule (reported FUSED_COMM / PEER), prcg_sync (blocking copy of pub_err
//                        on every call), prcg_iterate (consulted err_host), record() (waited for red_event), prcg_set_scalars
//                        (published / returned early), prcg_debug_layout (waves per workgroup)
//   red_pending,         the same sessions: record() and the tail of prcg_iterate
//   red_event
//   cg_one, cg_lag       after a one-launch Chronopoulos-Gear / Ghysels-Vanroose session, in every later session of another
//                        family: record() and the tail of prcg_iterate called cg_flush (a no-op only because cg_lag was false)
//   cg_fused             two-RHS sessions only cleared it by hand copy; now by the one reset
//   pr_q_valid           pipelined and Chronopoulos-Gear sessions: pr_unpack (guarded by pr_packed)
//   pend_parts, pend_k,  two-RHS sessions: not read there; every other family cleared them itself
//   pend_buf
//   rs_cur, q_cur, p_cur, cur_r, cur_s, cur_rt, cur_st, cur_w, cur_u, cur_t
//                        families that do not use a pointer kept the last session's; locate() and the *_args builders read
//                        only the ones their family sets
//   small_mode, xphase,  read only under flags their family sets; last_grid, last_wpb: prcg_debug_layout reported the last
//   last_grid, last_wpb  launch of an EARLIER session until the new one launched
struct Session {
    bool in_session = false;
    int variant = -1;
    bool prec = false;
    bool stored_tilde = false;   // M^-1 is a host callback or block Jacobi: every tilde vector is a stored vector
    bool bj_session = false;     // ... block Jacobi applies M^-1 in this session
    int max_iter = 0;
    int k = 0;
    uint32_t hist_mask = 0;
    bool have_xtrue = false;
    bool rhs2 = false;           // session type "two right-hand sides" (prcg_solve_begin_multi): Hestenes-Stiefel, or with
                                 // variant PRCG_PR / PRCG_M predict-and-recompute (two scalar / coefficient rows per iteration)
    int groups = 0;              // ... its PAIR GROUPS: 1 with two right-hand sides, 2 with four (group g: columns 2 g, 2 g + 1, a
                                 // complete two-RHS state of its own -- pair_group)
    bool spmm4 = false;          // ... two groups: the product of an iteration is ONE four-vector launch (sliced rows, PRCG_SPMM4)
    bool pipe2 = false;          // session type "pipelined predict-and-recompute, two right-hand sides" (prcg_solve_begin_multi_pipe):
                                 // rhs2 with one group, variant PRCG_PIPE_PR / PRCG_PIPE_PR_M, per column the pair arrays cxp, crs, cwu
                                 // (crst) around ONE product of four vectors (spmm4: in one launch); two scalar / coefficient rows per iteration
    // ---- schedule ----
    bool fused = false;          // pipelined: the one-launch-per-iteration kernel
    bool fused_comm = false;     // ... with a communicator: the interior launch waits in-kernel for the reduction
    bool peer = false;           // ... over the direct peer exchange
    bool gather = false;         // pipelined with a communicator: the merged exchange
    bool small = false;          // the one-workgroup solver (n <= 4096)
    int small_mode = 0;          // 0: matrix in LDS, 1: matrix in registers
    bool small_hs = false;       // Hestenes-Stiefel session of a small system: the whole solve in one launch of one workgroup
    bool hs_fused = false;       // Hestenes-Stiefel without reduction launches: 2 launches per iteration on window
                                 // operators (update; product with the direction formed in the staged window), else 3
    int hs_pend_mu = 0;          // ... mu of iteration pend_k exists only as this many block partials in partB
    bool pr_fused = false;       // non-pipelined predict-and-recompute (pr, m) on a window operator: ONE launch per iteration
                                 // (window formed as (z - a zs) + b p_old); z, zs, p double-buffered
    bool pr_packed = false;      // ... unpreconditioned, no per-iteration vector recorder: inside a prcg_iterate call the state lives PACKED,
                                 // one 32-byte entry (z, zs, p, x) per row in q / q2 (kEpiPROneQ: 16-byte accesses only); packed at the
                                 // call's first iteration, unpacked into r, s, p, x at its end
    bool pr_q_valid = false;     // ... the packed copy q_cur is the current state
    bool cg_fused = false;       // Chronopoulos-Gear / Ghysels-Vanroose on a window operator: two launches (product with the window formed as
                                 // r - a s; p, s update that sums the product's partials itself); r double-buffered (cur_r)
    bool cg_one = false;         // ... in ONE launch per iteration (launch_win_cg_one): the p, s (u) update of an iteration is deferred into the next
                                 // launch's window formation; s (cg) / t, u (gv) double-buffered as well
    bool cg_lag = false;         // ... and the update of iteration pend_k is pending (its partials: pend_buf / pend_parts)
    bool red_pending = false;    // fused_comm: the communication chain of the previous iteration is outstanding ...
    hipEvent_t red_event = nullptr;   // ... and this event marks its end
    int xphase = 0;              // deferred (x,p) store (FusedPrev::xphase): phase of the launch prcg_iterate issues next (0 outside its loop)
    // ---- which copy of a double-buffered vector is current ----
    double* rs_cur = nullptr;    // pipelined, one launch: the current SpMM input pairs: rs / rs2 ((r,s)), with Jacobi rst / rst2 ((r~,s~))
    double* q_cur = nullptr;     // pr_packed: q / q2
    double* p_cur = nullptr;     // the current direction: p / p2 (the product launch writes the other one)
    double* cur_r = nullptr; double* cur_s = nullptr; double* cur_rt = nullptr; double* cur_st = nullptr;
    double* cur_w = nullptr; double* cur_u = nullptr; double* cur_t = nullptr;
    // ---- inner products that exist only as block partials ----
    int pend_parts = 0;          // dots[pend_k] exist only as this many block partials ...
    int pend_k = -1;             // ... of iteration pend_k, in pend_buf
    double* pend_buf = nullptr;
    int last_grid = 0;           // workgroups of the session's last launch that left inner-product partials (prcg_debug_layout) ...
    int last_wpb = 0;            // ... and its waves per workgroup (window operators: what launch_win_v instantiated; else 0)
};

}  // namespace

// The resident operator (Operator) and the state of the open session (Session) are base sub-objects, so that each is a
// value of its own -- the operator's flags are assigned from the plan, the session is reset as a whole -- while the code
// below addresses their fields as before.
struct prcg_handle : Operator, Session {
    int dev = 0;
    std::string err;
    hipStream_t sc = nullptr;   // compute
    hipStream_t sm = nullptr;   // reductions + all-reduce
    hipStream_t sh = nullptr;   // halo exchange (own stream + own communicator: runs beside the all-reduce)
    hipEvent_t e_upd = nullptr, e_halo = nullptr, e_red = nullptr;
    hipEvent_t e_kdone = nullptr;   // completion signal of a launch itself (hipExtLaunchKernel), see FusedState::done
    hipEvent_t e_rdone = nullptr;   // ... of the unpack launch that ends the communication chain of an iteration

    Options opt;                // every PRCG_* switch (prcg_plan.h)

    // ---- communicator ----
    Rccl* rccl = nullptr;
    ncclComm_t comm = nullptr;    // all-reduce (and, if comm_halo is null, the halo too)
    ncclComm_t comm_halo = nullptr;
    int rank = 0, nranks = 1;

    // ---- halo plan ----
    int n_peers = 0;
    std::vector<int> peer_rank;
    std::vector<int64_t> send_ptr, recv_ptr;
    DevBuf send_idx, send_buf;
    bool have_halo = false;

    // ---- merged exchange: with a small halo, ONE all-gather per iteration carries the rank's five
    // partial inner products and the rows its neighbours need (pipelined variants; Session::gather) ----
    bool gather_planned = false, gather_ok = false;
    int g_slot = 0;                      // doubles per rank slot: 8 + 2 * (largest send list of any rank)
    DevBuf gbuf, ghost_src, gtab;

    // ---- allocations, reused from session to session by design (DevBuf::ensure) ----
    DevBuf tmp_ext;                      // 2*(n+g) doubles: SpMV input scratch with ghost room
    DevBuf t1;                           // 2*n doubles: SpMV output scratch
    DevBuf partA, partB;                 // block partials: update kernels / SpMV epilogues
    DevBuf partC;                        // one-launch schedules: second partials buffer (ping-pong with partB)
    DevBuf r2, s2, rt2, st2;     // one-launch predict-and-recompute: the second copies of r, s (r~, s~ with Jacobi)
    DevBuf x, xp, p, p2, rs, rs2, rst, rst2, wu, wt, wv, r, s, rt, st, b, xt, dinv, e_ext;
    DevBuf w, u, tvec;           // cg_cg / gv: w (ghost room), u, t = A w~
    DevBuf w2, u2, t2;           // ... their second copies (one- / two-launch schedules on window operators)
    DevBuf mx, mr, mp, ms, mrt;  // two right-hand sides: the interleaved n x 2 arrays X, R, P, S, RT (Hs2Args, prcg_kernels.h); dots / coef hold both columns per row
    DevBuf mst;                  // ... predict-and-recompute with Jacobi: ST (Pr2Args); dots / coef hold one row per column and iteration
    DevBuf mx1, mr1, mp1, ms1, mrt1, mst1;   // four right-hand sides: the same arrays of the SECOND pair group (columns 2, 3) ...
    DevBuf partA1, partB1;                   // ... and its block partials
    DevBuf x4b, y4b;             // prcg_spmm4: the second source / destination pair array (the first: tmp_ext / t1)
    DevBuf cxp[2], crs[2], cwu[2], crst[2];   // pipelined, two right-hand sides: column c's pairs (x,p), (r,s), (w,u) and with Jacobi (r~,s~) (Pipe2Args)
    DevBuf pub, pub_err;         // publication record of the reduced inner products / timeout flag
    DevBuf q, q2;                // packed predict-and-recompute state (Session::pr_packed)
    DevBuf dots, coef;
    void* placed_xp = nullptr;   // the (x,p) allocation that has been through place_session_vectors

    // preconditioners that are no diagonal scaling: sessions that use one run the schedules in which every tilde vector is
    // a stored vector (Session::stored_tilde).  Two kinds, the last one set is in force:
    //  * host callback (prcg_set_preconditioner): M^-1 v is computed by the caller's function on host copies of v;
    //  * point-block Jacobi (prcg_set_block_jacobi): M^-1 v is one launch of prcg_blockjac.hip on the compute stream
    prcg_prec_fn cb = nullptr; void* cb_ctx = nullptr;
    int bj_bs = 0; DevBuf bj_blocks;     // bj_bs > 0: blocks set, in the layout of block_jacobi_layout
    DevBuf bj_flag;                      // one int64: smallest index of a bad block of the last device build (prcg_build_block_jacobi)
    // ... or blocks of VARIABLE size (prcg_set_block_jacobi_var / prcg_build_block_jacobi_var): bj_var, then bj_bs == 0 and bj_blocks
    // holds prcg_bjvar.h's layout; the partition's tile table and lane bytes on the device, the partition itself on the host (getter)
    bool bj_var = false;
    BjVarPlan bjv_plan; std::vector<int64_t> bjv_ptr;
    DevBuf bjv_tiles, bjv_bytes;         // ntiles x 4 int64; code bytes (ntiles x 256) followed by block-in-tile bytes (ntiles x 256)
    bool have_block_jacobi() const { return bj_bs > 0 || bj_var; }
    const long long* bjv_tiles_d() const { return static_cast<const long long*>(bjv_tiles.p); }
    const unsigned char* bjv_code_d() const { return static_cast<const unsigned char*>(bjv_bytes.p); }
    const unsigned char* bjv_bidx_d() const { return bjv_code_d() + bjv_plan.ntiles * kBjvLanes; }
    prcg_replace_fn replace_fn = nullptr; void* replace_ctx = nullptr;       // gv_cg's w_replace predicate (prcg_set_replace_hook)
    std::vector<double> cb_in, cb_out;
    DevBuf cb_stage, ut;         // staging for strided operands; u~ = M^-1 u of the pipelined variants

    // ---- profiling ----
    int prof_stride = 0;
    std::vector<EventPair> ev_spmv, ev_upd;
    int n_ev_spmv = 0, n_ev_upd = 0;
    double last_tot_ms = 0.0;
    int64_t last_iters = 0;

    WinDev wdev() const { return Operator::wdev(opt.want_big); }
    // any communicator -- even a 1-rank one -- selects the two-stream schedule
    bool multi() const { return comm != nullptr; }

    // ---- direct peer exchange over xGMI (PeerDev, prcg_kernels.h): the multi-rank one-launch schedule without a collective ----
    void* xbuf = nullptr;                // this rank's exchange buffer
    size_t xbuf_bytes = 0;
    bool xbuf_fine = false;              // allocated fine-grained (what other GPUs' stores need); else plain device memory (one GPU)
    int ghost_cap = 0;                   // ghost rows per parity in EVERY rank's buffer (largest ghost count of any rank)
    std::vector<void*> peer_opened;      // other ranks' buffers opened with hipIpcOpenMemHandle
    PeerDev peer_host{};
    DevBuf peer_dev, peer_ents, peer_tile_send;
    bool peer_ok = false;                // connected: every rank's buffer is mapped, send entries planned
    uint64_t peer_epoch = 0;
    unsigned* err_host = nullptr;        // pinned host word a timed-out wave also writes: prcg_iterate sees it without a sync
    std::vector<int32_t> send_idx_host;  // prcg_set_halo's send lists (host copy: the peer plan is built from them)
    std::vector<int32_t> wt_rb, wt_re;   // rows of the window tiles in table order

    // every vector a window launch may stage (the pointer handed to the launch lies inside one of them)
    const DevBuf* owner(const void* ptr) const {
        const DevBuf* all[] = {&tmp_ext, &t1, &x, &xp, &p, &p2, &rs, &rs2, &rst, &rst2, &wu, &wt, &wv, &r, &r2, &s, &s2, &rt, &rt2,
                               &st, &st2, &b, &xt, &dinv, &e_ext, &w, &w2, &u, &u2, &tvec, &t2, &ut, &cb_stage, &q, &q2, &mx, &mp, &mx1, &mp1, &x4b,
                               &crs[0], &crs[1], &crst[0], &crst[1]};
        const char* c = static_cast<const char*>(ptr);
        for (const DevBuf* d : all)
            if (d->p && c >= static_cast<const char*>(d->p) && c < static_cast<const char*>(d->p) + d->bytes) return d;
        return nullptr;
    }
};

namespace {

int fail(prcg_t* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_last_error = buf;
    return code;
}

#define HIPCHK(h, expr)                                                                      \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess)                                                               \
            return fail(h, PRCG_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                        __FILE__, __LINE__);                                                 \
    } while (0)

#define NCCLCHK(h, expr)                                                                      \
    do {                                                                                      \
        ncclResult_t r__ = (expr);                                                            \
        if (r__ != ncclSuccess)                                                               \
            return fail(h, PRCG_ERCCL, "%s failed: %s (%s:%d)", #expr,                        \
                        (h)->rccl->GetErrorString(r__), __FILE__, __LINE__);                  \
    } while (0)

#define LAUNCHCHK(h, grid)                                                                    \
    do {                                                                                      \
        const int g__ = (grid);                                                               \
        if (g__ == -2) return PRCG_EINVAL;        /* refused by check_sources: message set */  \
        if (g__ < 0) return fail(h, PRCG_EHIP, "kernel launch failed (%s:%d)", __FILE__, __LINE__); \
    } while (0)

// the single-column accessors do not answer for column 0 of a two-RHS session
#define NOT_RHS2(h, name)                                                                     \
    CHECK(h, !(h)->rhs2, name ": the open session has two right-hand sides: it is read per column with "               \
                         "prcg_get_vector_rhs / _scalars_rhs / _coefficients_rhs / _history_rhs and has no setters")

#define CHECK(h, cond, ...)                                                                   \
    do { if (!(cond)) return fail(h, PRCG_EINVAL, __VA_ARGS__); } while (0)

// A window launch stages whole 64-column pages of its source vectors and the narrow column encodings of the
// CSR-adaptive kernels decode a few out-of-tile bytes per tile: every such source must hold its n + g entries AND
// kGatherPad spare ones behind them (prcg_window_source_ok).  Checked at every launch from the size of the
// allocation the pointer lies in -- a short source is an error code, not a memory fault.
int check_sources(prcg_t* h, std::initializer_list<std::pair<const void*, int>> srcs) {
    for (const auto& sc : srcs) {
        if (!sc.first) continue;
        const DevBuf* d = h->owner(sc.first);
        const int64_t avail = d ? (int64_t)(static_cast<const char*>(d->p) + d->bytes - static_cast<const char*>(sc.first)) : -1;
        if (!d || !prcg_window_source_ok(h->n, h->g, sc.second, avail))
            return fail(h, PRCG_EINVAL, "a matrix-product source vector holds %lld bytes, fewer than the %lld a launch over %lld rows + "
                        "%lld ghosts may touch (%d components, %d spare entries): launch refused",
                        (long long)avail, (long long)((h->n + h->g + kGatherPad) * (int64_t)sc.second * 8), (long long)h->n,
                        (long long)h->g, sc.second, kGatherPad);
    }
    return PRCG_OK;
}
#define SRCCHK(h, ...) do { if (check_sources(h, {__VA_ARGS__})) return -2; } while (0)              // inside a launch helper (returns a grid)
#define SRCCHK2(h, ...) do { if (check_sources(h, {__VA_ARGS__})) return PRCG_EINVAL; } while (0)   // inside an iterate_* function

// The matrix products of the engine: window kernels when the operator qualified, else sliced rows, else the
// CSR-adaptive tile kernels.  which: 0 = every tile, 1 = interior tiles, 2 = tiles touching ghosts.
struct TileRange { int first, count; };
TileRange tile_range(const prcg_t* h, int which) {
    const Operator& op = *h;
    const int n_int = op.win ? op.nwt_int : (op.sell ? op.nst_int : op.nt_int);
    const int n_bnd = op.win ? op.nwt_bnd : (op.sell ? op.nst_bnd : op.nt_bnd);
    return TileRange{which == 2 ? n_int : 0, which == 0 ? n_int + n_bnd : (which == 1 ? n_int : n_bnd)};
}
// (the narrow encodings of the CSR-adaptive tiles are per class: a launch over one class asks for that class's)
CsrDev csr_view(const prcg_t* h, int which) {
    return which == 0 ? h->csr() : (which == 1 ? h->csr(0, h->nt_bnd == 0) : h->csr(h->nt_int, false));
}
// The launch that left inner-product partials last -- what prcg_debug_layout reports: on a window operator the workgroups and
// waves per workgroup launch_win_v used (win_last_launch: call this right behind the launch), else the grid alone.
void note_partials_launch(prcg_t* h, int grid) {
    if (grid <= 0) return;
    const WinLaunchShape s = h->win ? win_last_launch() : WinLaunchShape{grid, 0};
    h->last_grid = s.grid; h->last_wpb = s.wpb;
}
int eng_spmv(prcg_t* h, hipStream_t st, int which, const double* x, double* y, SpmvEpilogue epi, const double* ep_r,
             const double* ep_d, double* ep_st, double* partials) {
    SRCCHK(h, {x, 1});
    const TileRange t = tile_range(h, which);
    if (h->win) {
        const int grid = launch_win_spmv(st, h->wdev(), h->wtile_ptr(t.first), t.count, h->win_geom, x, y, epi, ep_r, ep_d, ep_st, partials,
                                         h->opt.win_per_cu);
        if (epi != kEpiNone) note_partials_launch(h, grid);
        return grid;
    }
    const int grid = h->sell
        ? launch_sell_spmv(st, h->sdev(), h->sslice_ptr(t.first), t.count, x, y, epi, ep_r, ep_d, ep_st, partials, h->opt.sell_per_cu)
        : launch_spmv(st, csr_view(h, which), h->tile_ptr(t.first), t.count, h->steps, x, y, epi, ep_r, ep_d, ep_st, partials, h->opt.kn);
    if (epi != kEpiNone) note_partials_launch(h, grid);
    return grid;
}
int eng_spmm2(prcg_t* h, hipStream_t st, int which, const double* rs, double* wu, int mask) {
    SRCCHK(h, {rs, 2});
    const TileRange t = tile_range(h, which);
    if (h->win) return launch_win_spmm2(st, h->wdev(), h->wtile_ptr(t.first), t.count, h->win_geom, rs, wu, mask, h->opt.win_per_cu);
    if (h->sell) return launch_sell_spmm2(st, h->sdev(), h->sslice_ptr(t.first), t.count, rs, wu, mask, h->opt.sell_per_cu);
    return launch_spmm2(st, csr_view(h, which), h->tile_ptr(t.first), t.count, h->steps, rs, wu, mask, h->opt.kn);
}
// [dst0 | dst1] = A [src0 | src1], two pair arrays: one launch on sliced rows (PRCG_SPMM4=0: never), else a two-vector
// product per pair -- the same bits per column either way
bool spmm4_one_launch(const prcg_t* h) { return h->sell && h->opt.want_spmm4; }
int eng_spmm4(prcg_t* h, hipStream_t st, int which, const double* src0, const double* src1, double* dst0, double* dst1) {
    SRCCHK(h, {src0, 2}, {src1, 2});
    if (spmm4_one_launch(h)) {
        const TileRange t = tile_range(h, which);
        return launch_sell_spmm4(st, h->sdev(), h->sslice_ptr(t.first), t.count, src0, src1, dst0, dst1, h->opt.sell_per_cu);
    }
    const int g0 = eng_spmm2(h, st, which, src0, dst0, 3);
    if (g0 < 0) return g0;
    return eng_spmm2(h, st, which, src1, dst1, 3);
}
// (only the window kernels have the deferred form that runs one class of tiles; the others always take every tile)
int eng_fused(prcg_t* h, hipStream_t st, const FusedState& f, int which = 0) {
    SRCCHK(h, {f.in_old, 2});
    const TileRange t = tile_range(h, h->win ? which : 0);
    if (h->win)
        return launch_win_pipe_fused(st, h->wdev(), h->wtile_ptr(t.first), t.count, h->win_geom, f,
                                     f.deferred ? h->opt.defer_per_cu : h->opt.win_per_cu);
    if (h->sell) return launch_sell_pipe_fused(st, h->sdev(), h->sslice_ptr(t.first), t.count, f, h->opt.sell_per_cu);
    return launch_pipe_fused(st, h->csr(), h->tile_ptr(t.first), t.count, h->steps, f, h->opt.kn);
}

bool is_pipe(int v) { return v == PRCG_PIPE_PR || v == PRCG_PIPE_P || v == PRCG_PIPE_PR_M || v == PRCG_PIPE_P_M; }
bool is_pr(int v) { return v == PRCG_PR || v == PRCG_M; }
bool is_cg_family(int v) { return v == PRCG_CG_CG || v == PRCG_GV; }
bool pipe_recompute(int v) { return v == PRCG_PIPE_PR || v == PRCG_PIPE_PR_M; }
bool meurant(int v) { return v == PRCG_PIPE_PR_M || v == PRCG_PIPE_P_M || v == PRCG_M; }
// a recorder reads the state vectors after every iteration (so no schedule may leave them stale between two launches)
bool records_state(uint32_t hist_mask) {
    return (hist_mask & (PRCG_HIST_RESIDUAL_2_NORM | PRCG_HIST_ERROR_A_NORM | PRCG_HIST_ERROR_2_NORM)) != 0;
}

// ---- halo exchange of an nc-component extended vector, all on `st` ----------------------
int exchange(prcg_t* h, double* vec_ext, int nc, hipStream_t st) {
    // a rank takes part in the exchange if it has ghosts OR if a peer needs its rows (with a
    // pattern-symmetric operator the two coincide, but the plan decides, not the pattern)
    if (!h->multi()) return PRCG_OK;
    CHECK(h, h->g == 0 || h->have_halo, "matrix has ghost columns but prcg_set_halo was not called");
    if (!h->have_halo || h->n_peers == 0) return PRCG_OK;
    // the halo communicator is used on its own stream only
    ncclComm_t cm = (h->comm_halo && st == h->sh) ? h->comm_halo : h->comm;
    const int64_t nsend = h->send_ptr[h->n_peers];
    launch_pack(st, h->send_buf.d(), vec_ext, h->send_idx.i(), nsend, nc);
    NCCLCHK(h, h->rccl->GroupStart());
    ncclResult_t bad = ncclSuccess;
    for (int q = 0; q < h->n_peers && bad == ncclSuccess; ++q) {
        const int64_t ns = h->send_ptr[q + 1] - h->send_ptr[q];
        const int64_t nr = h->recv_ptr[q + 1] - h->recv_ptr[q];
        if (ns > 0)
            bad = h->rccl->Send(h->send_buf.d() + h->send_ptr[q] * nc, (size_t)(ns * nc), ncclDouble, h->peer_rank[q], cm, st);
        if (nr > 0 && bad == ncclSuccess)
            bad = h->rccl->Recv(vec_ext + (h->n + h->recv_ptr[q]) * nc, (size_t)(nr * nc), ncclDouble, h->peer_rank[q], cm, st);
    }
    // never leave the group open: a failed send/recv still gets its GroupEnd before the error is reported
    const ncclResult_t fin = h->rccl->GroupEnd();
    if (bad != ncclSuccess) return fail(h, PRCG_ERCCL, "ncclSend/ncclRecv failed: %s", h->rccl->GetErrorString(bad));
    NCCLCHK(h, fin);
    return PRCG_OK;
}

int allreduce(prcg_t* h, double* buf, int count, hipStream_t st) {
    if (!h->multi()) return PRCG_OK;
    NCCLCHK(h, h->rccl->AllReduce(buf, buf, (size_t)count, ncclDouble, ncclSum, h->comm, st));
    return PRCG_OK;
}

// Collective (every rank calls it, from prcg_solve_begin): is the halo small enough to ride
// on the reduction?  If so, learn where in each neighbour's slot this rank's ghost rows lie:
// the ranks all-gather their (peer, offset, count) send tables once.
int plan_gather(prcg_t* h) {
    if (!h->multi() || !h->opt.want_gather) return PRCG_OK;
    if (h->gather_planned) { h->gather = h->gather_ok; return PRCG_OK; }
    h->gather_planned = true;
    h->gather_ok = false;
    const int np = h->have_halo ? h->n_peers : 0;
    const int64_t nsend = np > 0 ? h->send_ptr[np] : 0;
    const int R = h->nranks;
    // (a) largest send list / peer count of any rank
    HIPCHK(h, h->gtab.alloc(2 * sizeof(double)));
    double mine[2] = {(double)nsend, (double)np}, mx[2] = {0, 0};
    HIPCHK(h, hipMemcpyAsync(h->gtab.p, mine, sizeof mine, hipMemcpyHostToDevice, h->sc));
    NCCLCHK(h, h->rccl->AllReduce(h->gtab.p, h->gtab.p, 2, ncclDouble, ncclMax, h->comm, h->sc));
    HIPCHK(h, hipMemcpyAsync(mx, h->gtab.p, sizeof mx, hipMemcpyDeviceToHost, h->sc));
    HIPCHK(h, hipStreamSynchronize(h->sc));
    const int64_t max_send = (int64_t)mx[0];
    const int max_peers = (int)mx[1];
    const int64_t slot = 8 + 2 * max_send;
    if (slot * (int64_t)sizeof(double) > h->opt.gather_max_bytes) return PRCG_OK;      // same verdict on every rank
    // (b) everybody's send table: [n_peers, (peer, first row of the list, rows) ...]
    const int T = 1 + 3 * max_peers;
    std::vector<double> tab((size_t)R * T, 0.0);
    double* my = tab.data() + (size_t)h->rank * T;
    my[0] = np;
    for (int q = 0; q < np; ++q) {
        my[1 + 3 * q] = h->peer_rank[q];
        my[2 + 3 * q] = (double)h->send_ptr[q];
        my[3 + 3 * q] = (double)(h->send_ptr[q + 1] - h->send_ptr[q]);
    }
    HIPCHK(h, h->gtab.alloc((size_t)R * T * sizeof(double)));
    HIPCHK(h, hipMemcpyAsync(h->gtab.d() + (size_t)h->rank * T, my, (size_t)T * sizeof(double), hipMemcpyHostToDevice, h->sc));
    NCCLCHK(h, h->rccl->AllGather(h->gtab.d() + (size_t)h->rank * T, h->gtab.p, (size_t)T, ncclDouble, h->comm, h->sc));
    HIPCHK(h, hipMemcpyAsync(tab.data(), h->gtab.p, tab.size() * sizeof(double), hipMemcpyDeviceToHost, h->sc));
    HIPCHK(h, hipStreamSynchronize(h->sc));
    // (c) ghost j  <-  pair index into the gathered buffer
    std::vector<int32_t> src((size_t)h->g + 1, 0);
    const int bad = plan_gather_sources(h->rank, T, tab.data(), np, h->peer_rank.data(), h->recv_ptr.data(), slot, src.data());
    CHECK(h, bad == 0, "halo plans disagree: rank %d sends no list of the expected length to rank %d (or index overflow)",
          bad > 0 ? h->peer_rank[bad - 1] : -1, h->rank);
    HIPCHK(h, h->ghost_src.alloc(src.size() * sizeof(int32_t)));
    HIPCHK(h, hipMemcpy(h->ghost_src.p, src.data(), src.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(h, h->gbuf.alloc((size_t)R * slot * sizeof(double)));
    HIPCHK(h, hipMemset(h->gbuf.p, 0, (size_t)R * slot * sizeof(double)));
    h->g_slot = (int)slot;
    h->gather_ok = true;
    h->gather = true;
    return PRCG_OK;
}

// y = A x (x extended, ghosts exchanged), everything on the compute stream.  Used by the
// initialisation, the recorders and prcg_spmv -- not by the timed loop.
int dist_spmv(prcg_t* h, double* x_ext, double* y, SpmvEpilogue epi, const double* ep_r,
              const double* ep_d, double* ep_st, int* grid_out) {
    int rc = exchange(h, x_ext, 1, h->sc);
    if (rc) return rc;
    const int grid = eng_spmv(h, h->sc, 0, x_ext, y, epi, ep_r, ep_d, ep_st, h->partB.d());
    LAUNCHCHK(h, grid);
    if (grid_out) *grid_out = grid;
    return PRCG_OK;
}

// the iterate x: second-class citizen of the pair array XP in the pipelined variants
const double* x_ptr(prcg_t* h) { return is_pipe(h->variant) ? h->xp.d() : h->x.d(); }
int x_stride(prcg_t* h) { return is_pipe(h->variant) ? 2 : 1; }

double* dots_at(prcg_t* h, int k) { return h->dots.d() + (size_t)k * kNS; }
double* coef_at(prcg_t* h, int k) { return h->coef.d() + (size_t)k * kCoefStride; }

void fused_flush(prcg_t* h);
void pr_unpack(prcg_t* h);
void hs_flush(prcg_t* h);
void cg_flush(prcg_t* h);
int flush_pending(prcg_t* h);
int apply_prec(prcg_t* h, const double* src, int sstride, double* dst, int dstride);

// ---- history recorders for the state of iteration k (compute stream) -------------------
int record(prcg_t* h, int k) {
    const uint32_t m = h->hist_mask;
    if (!records_state(m)) return PRCG_OK;
    int rc = flush_pending(h);      // the recorders reuse the partials buffers and read the state vectors
    if (rc) return rc;
    const int64_t n = h->n;
    if (m & PRCG_HIST_RESIDUAL_2_NORM) {
        // |b - A x|   callbacks/residual_2_norm.py:41
        launch_copy(h->sc, h->tmp_ext.d(), 1, x_ptr(h), x_stride(h), n);
        if ((rc = dist_spmv(h, h->tmp_ext.d(), h->t1.d(), kEpiNone, nullptr, nullptr, nullptr, nullptr))) return rc;
        const int grid = launch_diff_sq(h->sc, h->b.d(), 1, h->t1.d(), n, h->partA.d(), PRCG_S_RES2);
        LAUNCHCHK(h, grid);
        launch_reduce_final(h->sc, h->partA.d(), grid, dots_at(h, k), PRCG_S_RES2, PRCG_S_RES2, 1);
    }
    if (m & PRCG_HIST_ERROR_2_NORM) {
        // |x - x_true|   callbacks/error_2_norm.py:47-48
        const int grid = launch_diff_sq(h->sc, x_ptr(h), x_stride(h), h->xt.d(), n, h->partA.d(), PRCG_S_ERR2);
        LAUNCHCHK(h, grid);
        launch_reduce_final(h->sc, h->partA.d(), grid, dots_at(h, k), PRCG_S_ERR2, PRCG_S_ERR2, 1);
    }
    if (m & PRCG_HIST_ERROR_A_NORM) {
        // e = x - x_true; e'(A e)   callbacks/error_A_norm.py:47-48
        launch_sub(h->sc, h->e_ext.d(), 1, x_ptr(h), x_stride(h), h->xt.d(), 1, n);
        int grid = 0;
        // (a recorder's product, no inner product of the method: prcg_debug_layout keeps the iteration's launch)
        const int it_grid = h->last_grid, it_wpb = h->last_wpb;
        if ((rc = dist_spmv(h, h->e_ext.d(), h->t1.d(), kEpiDotXY, nullptr, nullptr, nullptr, &grid))) return rc;
        h->last_grid = it_grid; h->last_wpb = it_wpb;
        launch_reduce_final(h->sc, h->partB.d(), grid, dots_at(h, k), 0, PRCG_S_ERRA2, 1);
    }
    return allreduce(h, dots_at(h, k) + PRCG_S_RES2, 3, h->sc);
}

// `shift`: sample iteration k when k - shift is a multiple of the stride (see iterate_pipe_fused)
void prof_begin(prcg_t* h, std::vector<EventPair>& evs, int& count, int k, bool& on, int shift = 0) {
    on = h->prof_stride > 0 && ((k - shift) % h->prof_stride) == 0 && count < kMaxProfSamples;
    if (!on) return;
    if ((int)evs.size() <= count) {
        EventPair ep;
        if (hipEventCreate(&ep.a) != hipSuccess || hipEventCreate(&ep.b) != hipSuccess) { on = false; return; }
        evs.push_back(ep);
    }
    (void)hipEventRecord(evs[count].a, h->sc);
}
void prof_end(prcg_t* h, std::vector<EventPair>& evs, int& count, bool on) {
    if (!on) return;
    (void)hipEventRecord(evs[count].b, h->sc);
    ++count;
}

// SpMM of the pipelined loop.  The fixed-order reduction of the update kernel's block
// partials (and, with a communicator, the halo exchange and the one all-reduce) run on
// the communication stream, hidden behind the matrix product on the compute stream.
// `grid_upd` = number of partial blocks the update kernel just wrote to partA.
int pipe_spmm_and_reduce(prcg_t* h, int k, int grid_upd, bool profile) {
    double* in_ext = h->prec ? h->rst.d() : h->rs.d();
    const int mask = pipe_recompute(h->variant) ? 3 : 2;
    bool on = false;
    int rc;
    if (!h->multi()) {
        // everything in order on one stream
        launch_reduce_final(h->sc, h->partA.d(), grid_upd, dots_at(h, k), 0, 0, 5);
        if (profile) prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
        LAUNCHCHK(h, eng_spmm2(h, h->sc, 0, in_ext, h->wu.d(), mask));
        if (profile) prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
        if (h->bj_session) {
            // block Jacobi: both columns of [w u] in one launch that reads every block once
            if (h->bj_var)
                LAUNCHCHK(h, launch_block_jacobi_var_pair(h->sc, h->wt.d(), h->ut.d(), h->wu.d(), h->bjv_plan.ntiles, h->bjv_tiles_d(), h->bjv_code_d(),
                                                          h->bj_blocks.d(), mask));
            else
                LAUNCHCHK(h, launch_block_jacobi_pair(h->sc, h->wt.d(), h->ut.d(), h->wu.d(), h->n, h->bj_bs, h->bj_blocks.d(), mask));
        } else if (h->stored_tilde) {
            // u~ = preconditioner(u); w~ = preconditioner(w) in the flavours that recompute w (pipe_pr_cg.py:178-182)
            if ((rc = apply_prec(h, h->wu.d() + 1, 2, h->ut.d(), 1))) return rc;
            if (pipe_recompute(h->variant) && (rc = apply_prec(h, h->wu.d(), 2, h->wt.d(), 1))) return rc;
        }
        return PRCG_OK;
    }
    if (h->gather) {
        // small halo: pack (fixed-order reduction of the partials + the neighbours' rows) ->
        // ONE all-gather -> unpack (sums in rank order, ghost rows into place), all beside the
        // interior product
        const int np = h->have_halo ? h->n_peers : 0;
        double* slot = h->gbuf.d() + (size_t)h->rank * h->g_slot;
        HIPCHK(h, hipEventRecord(h->e_upd, h->sc));
        HIPCHK(h, hipStreamWaitEvent(h->sm, h->e_upd, 0));
        launch_gather_pack(h->sm, h->partA.d(), grid_upd, slot, in_ext, h->send_idx.i(), np > 0 ? (int)h->send_ptr[np] : 0);
        NCCLCHK(h, h->rccl->AllGather(slot, h->gbuf.p, (size_t)h->g_slot, ncclDouble, h->comm, h->sm));
        launch_gather_unpack(h->sm, h->gbuf.d(), h->g_slot, h->nranks, dots_at(h, k), in_ext + 2 * h->n,
                             h->ghost_src.i(), (int)h->g);
        HIPCHK(h, hipEventRecord(h->e_red, h->sm));
        if (profile) prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
        LAUNCHCHK(h, eng_spmm2(h, h->sc, 1, in_ext, h->wu.d(), mask));
        if (profile) prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
        HIPCHK(h, hipStreamWaitEvent(h->sc, h->e_red, 0));
        if (h->nt_bnd > 0) LAUNCHCHK(h, eng_spmm2(h, h->sc, 2, in_ext, h->wu.d(), mask));
        return PRCG_OK;
    }
    const bool halo = h->multi() && h->have_halo && h->n_peers > 0;
    HIPCHK(h, hipEventRecord(h->e_upd, h->sc));
    // With a halo communicator of its own the neighbour exchange runs on its own stream,
    // beside the reduction chain; with ONE communicator everything is one chain on the
    // reduction stream (halo first: the boundary rows need it before the next update needs
    // the inner products).
    hipStream_t hs = h->comm_halo ? h->sh : h->sm;
    HIPCHK(h, hipStreamWaitEvent(h->sm, h->e_upd, 0));
    if (halo) {
        if (hs != h->sm) HIPCHK(h, hipStreamWaitEvent(hs, h->e_upd, 0));
        if ((rc = exchange(h, in_ext, 2, hs))) return rc;
        HIPCHK(h, hipEventRecord(h->e_halo, hs));
    }
    // block partials -> 5 doubles -> the one all-reduce
    launch_reduce_final(h->sm, h->partA.d(), grid_upd, dots_at(h, k), 0, 0, 5);
    if ((rc = allreduce(h, dots_at(h, k), 5, h->sm))) return rc;
    HIPCHK(h, hipEventRecord(h->e_red, h->sm));

    if (profile) prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
    LAUNCHCHK(h, eng_spmm2(h, h->sc, 1, in_ext, h->wu.d(), mask));
    if (profile) prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
    if (halo) {
        HIPCHK(h, hipStreamWaitEvent(h->sc, h->e_halo, 0));
        LAUNCHCHK(h, eng_spmm2(h, h->sc, 2, in_ext, h->wu.d(), mask));
    }
    HIPCHK(h, hipStreamWaitEvent(h->sc, h->e_red, 0));
    return PRCG_OK;
}

// single-vector SpMV with an epilogue, interior rows overlapped with the halo of x_ext.
// partials of the two launches are laid end to end in partB; *nparts = their count.
int overlapped_spmv(prcg_t* h, int k, double* x_ext, double* y, SpmvEpilogue epi, const double* ep_r,
                    const double* ep_d, double* ep_st, int* nparts) {
    bool on = false;
    if (!h->multi()) {
        prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
        const int grid = eng_spmv(h, h->sc, 0, x_ext, y, epi, ep_r, ep_d, ep_st, h->partB.d());
        LAUNCHCHK(h, grid);
        prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
        *nparts = grid;
        return PRCG_OK;
    }
    hipStream_t hs = h->comm_halo ? h->sh : h->sm;
    HIPCHK(h, hipEventRecord(h->e_upd, h->sc));
    HIPCHK(h, hipStreamWaitEvent(hs, h->e_upd, 0));
    int rc = exchange(h, x_ext, 1, hs);
    if (rc) return rc;
    HIPCHK(h, hipEventRecord(h->e_halo, hs));
    prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
    const int g1 = eng_spmv(h, h->sc, 1, x_ext, y, epi, ep_r, ep_d, ep_st, h->partB.d());
    LAUNCHCHK(h, g1);
    prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
    HIPCHK(h, hipStreamWaitEvent(h->sc, h->e_halo, 0));
    const int g2 = eng_spmv(h, h->sc, 2, x_ext, y, epi, ep_r, ep_d, ep_st, h->partB.d() + (size_t)g1 * kPartialStride);
    LAUNCHCHK(h, g2);
    *nparts = g1 + g2;
    return PRCG_OK;
}

PipeUpdateArgs pipe_args(prcg_t* h, int k) {
    PipeUpdateArgs a{};
    a.n = h->n;
    a.xp = h->xp.d();
    a.rs = h->rs.d(); a.rst = h->prec ? h->rst.d() : nullptr;
    a.wu = h->wu.d(); a.wt = h->wt.d();
    a.d = (h->prec && !h->stored_tilde) ? h->dinv.d() : nullptr;
    a.ut = h->stored_tilde ? h->ut.d() : nullptr;
    a.dots_prev = k > 0 ? dots_at(h, k - 1) : dots_at(h, 0);
    a.coef_out = coef_at(h, k);
    a.partials = h->partA.d();
    a.meurant = meurant(h->variant);
    a.recompute_w = pipe_recompute(h->variant);
    return a;
}

// One launch per iteration (single GPU, all four pipelined flavours, with or without Jacobi): state k-1 =
// {XP, the SpMM input pairs in rs_cur, dots[k-1]} (+ (r,s) with Jacobi, + w (w~) for the 'p' flavours); the
// kernel computes A [in.x in.y] row by row and applies update k to the row at once.  The reduction of the inner products is NOT
// overlapped with anything here (it is needed at the head of the next launch) -- which is
// why ranks with a communicator keep the two-kernel schedule below.
// make dots[pend_k] real if the last fused launch left it as block partials
void fused_flush(prcg_t* h) {
    if (h->pend_parts > 0) {
        launch_reduce_final(h->sc, h->pend_buf, h->pend_parts, dots_at(h, h->pend_k), 0, 0, 5);
        h->pend_parts = 0;
    }
}

// The session runs the deferred (x,p) store: single GPU, window operator, no recorder that reads x between two launches
// of one prcg_iterate call.  A property of the open session: PRCG_XP_DEFER is fixed once the operator is set
// (prcg_set_option refuses it after prcg_set_csr), and the arrays in memory are current outside prcg_iterate's loop.
bool xp_deferred(const prcg_t* h) {
    const Session& s = *h;
    return h->opt.want_xp_defer && s.in_session && is_pipe(s.variant) && s.fused && !s.fused_comm && !s.small && h->win && !h->multi() &&
           !records_state(s.hist_mask);
}

// what both one-launch pipelined schedules hand their kernel: the state of iteration k-1 and where iteration k goes
FusedState fused_state(prcg_t* h, int k, double* in_old, double* in_new, double* part_out) {
    const bool rec = pipe_recompute(h->variant), prec = h->prec;
    FusedState f{};
    f.in_old = in_old; f.in_new = in_new; f.xp = h->xp.d();
    f.rs = prec ? h->rs.d() : nullptr;
    f.dinv = prec ? h->dinv.d() : nullptr;
    f.w = rec ? nullptr : h->wv.d();
    f.wt = (!rec && prec) ? h->wt.d() : nullptr;
    f.dots_prev = dots_at(h, k - 1); f.coef_out = coef_at(h, k); f.partials = part_out;
    f.meurant = meurant(h->variant); f.recompute_w = rec;
    return f;
}

int iterate_pipe_fused(prcg_t* h, int k) {
    double* const bufA = h->prec ? h->rst.d() : h->rs.d();
    double* const bufB = h->prec ? h->rst2.d() : h->rs2.d();
    double* rs_old = h->rs_cur;
    double* rs_new = (h->rs_cur == bufA) ? bufB : bufA;
    // partials of iteration k-1 (if still pending) are consumed by this launch's prologue
    FusedPrev prev{nullptr, 0, nullptr, nullptr, nullptr, nullptr};
    if (h->pend_parts > 0 && h->pend_k == k - 1) {
        prev = FusedPrev{h->pend_buf, h->pend_parts, dots_at(h, k - 1), nullptr, nullptr, nullptr};
    } else {
        fused_flush(h);
    }
    double* part_out = (h->pend_buf == h->partB.d()) ? h->partC.d() : h->partB.d();
    bool on = false;
    // SKIP and APPLY launches alternate: with an even sampling stride every sample would meet the same phase, so every
    // second sample is taken one launch later -- the mean launch time is then the mean of both phases
    const int ps = h->prof_stride;
    prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on, (h->xphase != 0 && ps > 0 && ps % 2 == 0) ? ((k / ps) & 1) : 0);
    FusedState f = fused_state(h, k, rs_old, rs_new, part_out);
    f.stream_stores = h->stream_stores;
    f.prev = prev;
    f.prev.xphase = h->xphase;
    f.prev.xcoef = h->xphase == 2 ? coef_at(h, k - 1) : nullptr;
    const int grid = eng_fused(h, h->sc, f);
    LAUNCHCHK(h, grid);
    prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
    h->pend_parts = grid; h->pend_k = k; h->pend_buf = part_out;
    note_partials_launch(h, grid);
    h->rs_cur = rs_new;
    return PRCG_OK;
}

// One launch per iteration WITH a communicator (window operators): the GPU form of
// VecDotBegin ... KSP_MatMult ... VecDotEnd (scaling_experiments_petsc/cg_impls/pipeprcg.c:154-173).
//
//   compute stream : [launch k: every wave: products of its first interior tiles | wait pub >= k-1 | their updates |
//                     remaining tiles fused, the tiles that touch ghost rows last] [launch k+1 ...          (back to back)
//   comm stream    : wait "launch k done" -> [pack partials + rows] [ncclAllGather] [unpack: dots[k], ghosts of
//                     (r,s)_k into place, release, publish k]
//
// The reduction AND the halo of iteration k travel while launch k+1 computes A [r s] on interior rows -- the overlap
// the two-kernel schedule has, without storing (w,u), without a separate update launch, without a second launch for
// the boundary rows and without any wait of the compute stream on the communication stream: the only
// synchronisation the compute stream sees is inside the kernel.
int iterate_pipe_fused_comm(prcg_t* h, int k) {
    double* const bufA = h->prec ? h->rst.d() : h->rs.d();
    double* const bufB = h->prec ? h->rst2.d() : h->rs2.d();
    double* in_old = h->rs_cur;
    double* in_new = (h->rs_cur == bufA) ? bufB : bufA;
    double* part_out = (k & 1) ? h->partB.d() : h->partC.d();
    FusedState f = fused_state(h, k, in_old, in_new, part_out);
    // (the deferred form gains nothing from streaming stores where the plain schedule gains 20 % -- S3 on one rank 143.7 against
    //  142.7 us -- and loses 13 % where the vectors just exceed the Infinity Cache -- one half of S3: 78.1 against 68.0 us;
    //  profiles/r04_sweeps.md: plain stores unless PRCG_STREAM_STORES=1 asks)
    f.stream_stores = h->opt.stream_override > 0 ? 1 : 0;
    f.prev = FusedPrev{};
    f.prev.pub = h->pub.d(); f.prev.want = (unsigned)(k - 1); f.prev.err = static_cast<unsigned*>(h->pub_err.p);
    f.deferred = 1;
    f.prev.nt_int = h->nwt_int;
    // ONE launch over all tiles: the boundary tiles come last in the table and are touched only after the wave has
    // seen the publication (which the ghost rows precede).  The launch signals the communication stream with its own
    // completion (no marker packet on the compute stream: the next iteration's launch follows directly).
    const bool ext_signal = h->opt.ext_signal && !h->peer;
    f.done = ext_signal ? h->e_kdone : nullptr;
    if (h->peer) {
        // direct peer exchange: this launch is the whole iteration -- its tiles send the neighbours' rows, its last workgroup
        // this rank's partial sums, and its workgroup 0 turns the ranks' slots of iteration k-1 into the publication
        f.prev.px = static_cast<const PeerDev*>(h->peer_dev.p);
        f.prev.dots_prev_out = dots_at(h, k - 1);
        f.prev.err_host = h->err_host;
        // the partial sums launch k-1 left are summed and SENT by this launch's communication wave (none pending: the
        // slot of iteration k-1 is already out -- session start, teacher forcing, or the end of the last prcg_iterate call)
        if (h->pend_parts > 0 && h->pend_k == k - 1) { f.prev.prev_partials = h->pend_buf; f.prev.nprev = h->pend_parts; }
    }
    bool on = false;
    prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
    const int g1 = eng_fused(h, h->sc, f, 0);
    LAUNCHCHK(h, g1);
    note_partials_launch(h, g1);
    prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
    if (h->peer) {
        h->pend_parts = g1; h->pend_k = k; h->pend_buf = part_out;
        h->rs_cur = in_new;
        return PRCG_OK;
    }
    const int g2 = 0;
    if (ext_signal) {
        HIPCHK(h, hipStreamWaitEvent(h->sm, h->e_kdone, 0));
    } else {
        HIPCHK(h, hipEventRecord(h->e_upd, h->sc));
        HIPCHK(h, hipStreamWaitEvent(h->sm, h->e_upd, 0));
    }
    const int nparts = g1 + g2;
    int rc;
    if (h->gather) {
        const int np = h->have_halo ? h->n_peers : 0;
        double* slot = h->gbuf.d() + (size_t)h->rank * h->g_slot;
        launch_gather_pack(h->sm, part_out, nparts, slot, in_new, h->send_idx.i(), np > 0 ? (int)h->send_ptr[np] : 0);
        NCCLCHK(h, h->rccl->AllGather(slot, h->gbuf.p, (size_t)h->g_slot, ncclDouble, h->comm, h->sm));
        launch_gather_unpack(h->sm, h->gbuf.d(), h->g_slot, h->nranks, dots_at(h, k), in_new + 2 * h->n, h->ghost_src.i(),
                             (int)h->g, h->pub.d(), (unsigned)k, ext_signal ? h->e_rdone : nullptr);
        if (!ext_signal) HIPCHK(h, hipEventRecord(h->e_red, h->sm));
        h->red_event = ext_signal ? h->e_rdone : h->e_red;
    } else {
        if (h->have_halo && h->n_peers > 0 && (rc = exchange(h, in_new, 2, h->sm))) return rc;
        launch_reduce_final(h->sm, part_out, nparts, dots_at(h, k), 0, 0, 5);
        if ((rc = allreduce(h, dots_at(h, k), 5, h->sm))) return rc;
        launch_publish(h->sm, dots_at(h, k), h->pub.d(), (unsigned)k);
        HIPCHK(h, hipEventRecord(h->e_red, h->sm));
        h->red_event = h->e_red;
    }
    h->red_pending = true;
    h->rs_cur = in_new;
    return PRCG_OK;
}

int iterate_pipe(prcg_t* h, int k) {
    // pipe_pr_cg.py:61-75 / :169-187
    if (h->fused_comm) return iterate_pipe_fused_comm(h, k);
    if (h->fused) return iterate_pipe_fused(h, k);
    PipeUpdateArgs a = pipe_args(h, k);
    bool on = false;
    prof_begin(h, h->ev_upd, h->n_ev_upd, k, on);
    const int grid = launch_pipe_update(h->sc, a);
    LAUNCHCHK(h, grid);
    prof_end(h, h->ev_upd, h->n_ev_upd, on);
    return pipe_spmm_and_reduce(h, k, grid, true);
}

HsArgs hs_args(prcg_t* h, int k) {
    HsArgs a{};
    a.n = h->n;
    a.x = h->x.d(); a.r = h->r.d(); a.rt = h->prec ? h->rt.d() : nullptr;
    a.p = h->p_cur; a.s = h->s.d(); a.d = (h->prec && !h->stored_tilde) ? h->dinv.d() : nullptr;
    a.dots_prev = k > 0 ? dots_at(h, k - 1) : dots_at(h, 0);
    a.dots_cur = dots_at(h, k);
    a.coef_out = coef_at(h, k);
    a.partials = h->partA.d();
    return a;
}

int iterate_hs(prcg_t* h, int k) {
    // hs_cg.py:54-61: two dependent reductions per iteration -- nothing to overlap them with
    HsArgs a = hs_args(h, k);
    bool on = false;
    prof_begin(h, h->ev_upd, h->n_ev_upd, k, on);
    const int g1 = launch_hs_update_xr(h->sc, a);
    LAUNCHCHK(h, g1);
    prof_end(h, h->ev_upd, h->n_ev_upd, on);
    launch_reduce_final(h->sc, h->partA.d(), g1, dots_at(h, k), PRCG_S_NU, PRCG_S_NU, 2);
    int rc;
    if (h->stored_tilde) {
        // r~ = preconditioner(r) -- host callback or block-Jacobi launch (hs_pcg :118) --, then nu = r~.r as an inner product of its own
        if ((rc = apply_prec(h, h->r.d(), 1, h->rt.d(), 1))) return rc;
        const int g2 = launch_dot(h->sc, h->rt.d(), h->r.d(), h->n, h->partB.d(), 0);
        LAUNCHCHK(h, g2);
        launch_reduce_final(h->sc, h->partB.d(), g2, dots_at(h, k), 0, PRCG_S_NU, 1);
    }
    rc = allreduce(h, dots_at(h, k) + PRCG_S_NU, 2, h->sc);              // reduction 1: nu
    if (rc) return rc;
    LAUNCHCHK(h, launch_hs_update_p(h->sc, a));
    int nparts = 0;
    if ((rc = overlapped_spmv(h, k, h->p_cur, h->s.d(), kEpiDotXY, nullptr, nullptr, nullptr, &nparts))) return rc;
    launch_reduce_final(h->sc, h->partB.d(), nparts, dots_at(h, k), 0, PRCG_S_MU, 1);
    return allreduce(h, dots_at(h, k) + PRCG_S_MU, 1, h->sc);           // reduction 2: mu
}

// make mu of iteration pend_k real if the last product launch left it as block partials
void hs_flush(prcg_t* h) {
    if (h->hs_pend_mu > 0) {
        launch_reduce_final(h->sc, h->partB.d(), h->hs_pend_mu, dots_at(h, h->pend_k), 0, PRCG_S_MU, 1);
        h->hs_pend_mu = 0;
    }
}

// Two right-hand sides in one Hestenes-Stiefel session (hs_cg.py:54-62 / hs_pcg :116-125 for each column): the vector
// kernels of prcg_rhs2.hip around ONE two-vector product of [p_0 p_1] -- the operator is streamed once for both systems.
// Four right-hand sides are two PAIR GROUPS, each a complete state of this kind (its own arrays, block partials and rows of
// dots / coef: group g's rows follow group g - 1's max_iter + 1 iterations), around ONE product of both groups' directions.
bool pr2(const prcg_t* h) { return h->rhs2 && is_pr(h->variant); }
// the session keeps one scalar and one coefficient row per column and iteration, each in the single-session order
bool two_rows(const prcg_t* h) { return pr2(h) || h->pipe2; }
struct PairGroup { DevBuf *x, *r, *p, *s, *rt, *st, *partA, *partB; int row0; };
PairGroup pair_group(prcg_t* h, int g) {
    const int row0 = g * (h->max_iter + 1) * (pr2(h) ? 2 : 1);
    if (g == 0) return PairGroup{&h->mx, &h->mr, &h->mp, &h->ms, &h->mrt, &h->mst, &h->partA, &h->partB, row0};
    return PairGroup{&h->mx1, &h->mr1, &h->mp1, &h->ms1, &h->mrt1, &h->mst1, &h->partA1, &h->partB1, row0};
}
// s = A p of every column: one two-vector product, or with two pair groups one product of [P_0 P_1 | P_2 P_3]
int multi_product(prcg_t* h, int k) {
    bool on = false;
    prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
    if (h->groups == 2) LAUNCHCHK(h, eng_spmm4(h, h->sc, 0, h->mp.d(), h->mp1.d(), h->ms.d(), h->ms1.d()));
    else LAUNCHCHK(h, eng_spmm2(h, h->sc, 0, h->mp.d(), h->ms.d(), 3));
    prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
    return PRCG_OK;
}
Hs2Args hs2_args(prcg_t* h, int k, int g) {
    const PairGroup G = pair_group(h, g);
    Hs2Args a{};
    a.n = h->n;
    a.x = G.x->d(); a.r = G.r->d(); a.rt = h->prec ? G.rt->d() : nullptr; a.p = G.p->d(); a.s = G.s->d();
    a.d = h->prec ? h->dinv.d() : nullptr;
    a.dots_prev = k > 0 ? dots_at(h, G.row0 + k - 1) : nullptr;
    a.dots_cur = dots_at(h, G.row0 + k);
    a.coef_out = coef_at(h, G.row0 + k);
    a.partials = G.partA->d();
    return a;
}
// s = A p for every column, then per group mu_c = p.s (a launch of its own: the multi-vector products have no dot epilogue)
int hs2_product_and_mu(prcg_t* h, int k) {
    int rc = multi_product(h, k);
    if (rc) return rc;
    for (int g = 0; g < h->groups; ++g) {
        const PairGroup G = pair_group(h, g);
        Hs2Args a = hs2_args(h, k, g);
        a.partials = G.partB->d();
        const int grid = launch_hs2_dot_ps(h->sc, a);
        LAUNCHCHK(h, grid);
        launch_reduce_final(h->sc, G.partB->d(), grid, dots_at(h, G.row0 + k), kHs2Mu, kHs2Mu, 2);
    }
    return PRCG_OK;
}
int iterate_hs2(prcg_t* h, int k) {
    for (int g = 0; g < h->groups; ++g) {
        const Hs2Args a = hs2_args(h, k, g);
        bool on = false;
        if (g == 0) prof_begin(h, h->ev_upd, h->n_ev_upd, k, on);             // (the sample: the first group's update launch)
        const int g1 = launch_hs2_update_xr(h->sc, a);
        LAUNCHCHK(h, g1);
        prof_end(h, h->ev_upd, h->n_ev_upd, on);
        launch_reduce_final(h->sc, a.partials, g1, dots_at(h, pair_group(h, g).row0 + k), kHs2Nu, kHs2Nu, 4);     // nu_0, rr_0, nu_1, rr_1
        LAUNCHCHK(h, launch_hs2_update_p(h->sc, a));
    }
    return hs2_product_and_mu(h, k);
}

// Two right-hand sides in one predict-and-recompute session (pr_cg.py:146-158 for each column; PRCG_M: Meurant's prediction):
// update, ONE two-vector product of [p_0 p_1], the three inner products that need s, one reduction launch per column.
Pr2Args pr2_args(prcg_t* h, int k, int g) {
    const PairGroup G = pair_group(h, g);
    Pr2Args a{};
    a.n = h->n;
    a.x = G.x->d(); a.r = G.r->d(); a.p = G.p->d(); a.s = G.s->d();
    a.rt = h->prec ? G.rt->d() : nullptr; a.st = h->prec ? G.st->d() : nullptr;
    a.d = h->prec ? h->dinv.d() : nullptr;
    a.dots_prev = k > 0 ? dots_at(h, G.row0 + 2 * (k - 1)) : nullptr;       // rows 2 (k - 1), 2 (k - 1) + 1: the columns' sums of k - 1
    a.coef_out = coef_at(h, G.row0 + 2 * k);
    a.part0 = G.partA->d(); a.part1 = G.partB->d();
    a.meurant = meurant(h->variant);
    return a;
}
// s = A p for every column, (s~ = d s), mu, dl, gm; then the five sums of each column: rows 2 k and 2 k + 1 of its group
// (g_upd[g]: the grid of group g's update launch, whose partials the sums include)
int pr2_product_and_sums(prcg_t* h, int k, const int* g_upd) {
    int rc = multi_product(h, k);
    if (rc) return rc;
    for (int g = 0; g < h->groups; ++g) {
        const Pr2Args a = pr2_args(h, k, g);
        const int grid = launch_pr2_dots(h->sc, a);
        LAUNCHCHK(h, grid);
        CHECK(h, grid == g_upd[g], "two-RHS session: the update and the dots launch disagree on the grid (%d, %d)", g_upd[g], grid);
        const int row = pair_group(h, g).row0 + 2 * k;
        launch_reduce_final(h->sc, a.part0, grid, dots_at(h, row), 0, 0, 5);
        launch_reduce_final(h->sc, a.part1, grid, dots_at(h, row + 1), 0, 0, 5);
    }
    return PRCG_OK;
}
int iterate_pr2(prcg_t* h, int k) {
    int g_upd[2] = {0, 0};
    for (int g = 0; g < h->groups; ++g) {
        const Pr2Args a = pr2_args(h, k, g);
        bool on = false;
        if (g == 0) prof_begin(h, h->ev_upd, h->n_ev_upd, k, on);             // (the sample: the first group's update launch)
        g_upd[g] = launch_pr2_update(h->sc, a);
        LAUNCHCHK(h, g_upd[g]);
        prof_end(h, h->ev_upd, h->n_ev_upd, on);
    }
    return pr2_product_and_sums(h, k, g_upd);
}

// Two right-hand sides in one pipelined predict-and-recompute session (pipe_pr_cg.py:61-75 / :169-187 for each column; the
// flavours that recompute w): ONE update launch for both columns, one reduction launch per column, ONE product of four vectors
// [w_0 u_0 | w_1 u_1] = A [r_0 s_0 | r_1 s_1] (with Jacobi of the (r~,s~) pairs) -- the operator is streamed once for both systems.
Pipe2Args pipe2_args(prcg_t* h, int k) {
    Pipe2Args a{};
    a.n = h->n;
    for (int c = 0; c < 2; ++c) {
        a.xp[c] = h->cxp[c].d(); a.rs[c] = h->crs[c].d(); a.wu[c] = h->cwu[c].d();
        a.rst[c] = h->prec ? h->crst[c].d() : nullptr;
    }
    a.d = h->prec ? h->dinv.d() : nullptr;
    a.dots_prev = k > 0 ? dots_at(h, 2 * (k - 1)) : nullptr;                // rows 2 (k - 1), 2 (k - 1) + 1: the columns' sums of k - 1
    a.coef_out = coef_at(h, 2 * k);
    a.part0 = h->partA.d(); a.part1 = h->partB.d();
    a.meurant = meurant(h->variant);
    return a;
}
// the five sums of each column from the block partials an update (or dots) launch of `grid` blocks left: rows 2 k, 2 k + 1
void pipe2_reduce(prcg_t* h, int k, int grid) {
    launch_reduce_final(h->sc, h->partA.d(), grid, dots_at(h, 2 * k), 0, 0, 5);
    launch_reduce_final(h->sc, h->partB.d(), grid, dots_at(h, 2 * k + 1), 0, 0, 5);
}
// (w_c, u_c) = A (r_c, s_c) of both columns (Jacobi: A (r~_c, s~_c)): one launch on sliced rows, else two two-vector launches
int pipe2_product(prcg_t* h) {
    DevBuf* src = h->prec ? h->crst : h->crs;
    LAUNCHCHK(h, eng_spmm4(h, h->sc, 0, src[0].d(), src[1].d(), h->cwu[0].d(), h->cwu[1].d()));
    return PRCG_OK;
}
int iterate_pipe2(prcg_t* h, int k) {
    const Pipe2Args a = pipe2_args(h, k);
    bool on = false;
    prof_begin(h, h->ev_upd, h->n_ev_upd, k, on);
    const int grid = launch_pipe2_update(h->sc, a);
    LAUNCHCHK(h, grid);
    prof_end(h, h->ev_upd, h->n_ev_upd, on);
    pipe2_reduce(h, k, grid);
    prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
    const int rc = pipe2_product(h);
    if (rc) return rc;
    prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
    return PRCG_OK;
}

// hs_cg.py:54-62 (hs_pcg :116-125) on one GPU without reduction launches.  The two inner products still separate
// the iteration into two phases (that IS Hestenes-Stiefel), but each phase's block partials are summed by every
// workgroup of the NEXT launch (same fixed order everywhere):
//   launch 1  [mu_k1 from the product's partials; a = nu_k1 / mu_k1]  x += a p;  r -= a s;  (r~ = d r);  nu_k partials
//   launch 2  [nu_k from launch 1's partials; b = nu_k / nu_k1]  window operators: p = z + b p_old formed while the
//             input window is staged, s = A p, mu_k partials, p_k written to the other direction buffer;
//             CSR-adaptive tiles: the p update (with that prologue) and the product are two launches.
int iterate_hs_fused(prcg_t* h, int k) {
    HsArgs a = hs_args(h, k);
    const bool have_mu = h->hs_pend_mu > 0 && h->pend_k == k - 1;
    if (!have_mu) hs_flush(h);
    bool on = false;
    prof_begin(h, h->ev_upd, h->n_ev_upd, k, on);
    const int g1 = launch_hs_update_xr(h->sc, a, have_mu ? h->partB.d() : nullptr, have_mu ? h->hs_pend_mu : 0, dots_at(h, k - 1));
    LAUNCHCHK(h, g1);
    prof_end(h, h->ev_upd, h->n_ev_upd, on);
    h->hs_pend_mu = 0;
    int grid = 0;
    on = false;
    if (h->win) {
        FusedPrev hs{};
        hs.prev_partials = h->partA.d(); hs.nprev = g1;
        hs.dots_prev_out = dots_at(h, k); hs.dots_old = dots_at(h, k - 1);
        double* p_new = (h->p_cur == h->p.d()) ? h->p2.d() : h->p.d();
        SRCCHK2(h, {h->prec ? h->rt.d() : h->r.d(), 1}, {h->p_cur, 1});
        prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
        grid = launch_win_hs(h->sc, h->wdev(), h->wtile_ptr(0), h->nwt_int + h->nwt_bnd, h->win_geom,
                             h->prec ? h->rt.d() : h->r.d(), h->p_cur, p_new, h->s.d(), h->partB.d(), coef_at(h, k), hs,
                             h->opt.win_per_cu);
        LAUNCHCHK(h, grid);
        note_partials_launch(h, grid);
        prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
        h->p_cur = p_new;
    } else {
        LAUNCHCHK(h, launch_hs_update_p(h->sc, a, h->partA.d(), g1, dots_at(h, k)));
        prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
        grid = eng_spmv(h, h->sc, 0, h->p_cur, h->s.d(), kEpiDotXY, nullptr, nullptr, nullptr, h->partB.d());
        LAUNCHCHK(h, grid);
        prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
    }
    h->hs_pend_mu = grid; h->pend_k = k;
    return PRCG_OK;
}

// pr_cg.py:146-158 (pr_pcg, m_pcg) in ONE launch per iteration on a window operator (launch_win_pr_one): the
// partials of launch k-1 are summed by every workgroup of launch k (as in iterate_pipe_fused), a and b follow,
// the staged window of the new direction is formed from the old r~ (r), s~ (s), p, and the row's own vectors and
// the five partials are written by the lane that summed the row.  r~ / s~ / p (r / s / p without Jacobi) are
// double-buffered: other tiles still stage the old values.
int iterate_pr_fused(prcg_t* h, int k) {
    const bool jac = h->prec;
    double*& z_cur = jac ? h->cur_rt : h->cur_r;
    double*& zs_cur = jac ? h->cur_st : h->cur_s;
    double* z_a = jac ? h->rt.d() : h->r.d();   double* z_b = jac ? h->rt2.d() : h->r2.d();
    double* zs_a = jac ? h->st.d() : h->s.d();  double* zs_b = jac ? h->st2.d() : h->s2.d();
    double* z_new = (z_cur == z_a) ? z_b : z_a;
    double* zs_new = (zs_cur == zs_a) ? zs_b : zs_a;
    double* p_new = (h->p_cur == h->p.d()) ? h->p2.d() : h->p.d();
    FusedPrev f{};
    if (h->pend_parts > 0 && h->pend_k == k - 1) {
        f.prev_partials = h->pend_buf; f.nprev = h->pend_parts; f.dots_prev_out = dots_at(h, k - 1);
    } else {
        fused_flush(h);
    }
    f.dots_old = dots_at(h, k - 1);
    f.pr.z_old = z_cur; f.pr.zs_old = zs_cur; f.pr.p_old = h->p_cur;
    f.pr.z_new = z_new; f.pr.zs_new = zs_new; f.pr.p_new = p_new;
    f.pr.x = h->x.d();
    f.pr.r = jac ? h->r.d() : nullptr; f.pr.s = jac ? h->s.d() : nullptr; f.pr.d = jac ? h->dinv.d() : nullptr;
    if (h->pr_packed) {
        // the state as 16-byte pairs (z, zs) and (p, x): packed once per prcg_iterate call (pr_unpack at its end); each of q / q2
        // holds the (z, zs) pairs with ghost room and spare entries, then the (p, x) pairs
        const size_t half = (size_t)2 * (h->n + h->g + kGatherPad);
        if (!h->pr_q_valid) {
            h->q_cur = h->q.d();
            launch_copy(h->sc, h->q_cur + 0, 2, z_cur, 1, h->n);
            launch_copy(h->sc, h->q_cur + 1, 2, zs_cur, 1, h->n);
            launch_copy(h->sc, h->q_cur + half + 0, 2, h->p_cur, 1, h->n);
            launch_copy(h->sc, h->q_cur + half + 1, 2, h->x.d(), 1, h->n);
            h->pr_q_valid = true;
        }
        double* q_other = (h->q_cur == h->q.d()) ? h->q2.d() : h->q.d();
        f.pr.q_old = h->q_cur; f.pr.px_old = h->q_cur + half;
        f.pr.q_new = q_other; f.pr.px_new = q_other + half;
    }
    double* part_out = (h->pend_buf == h->partB.d()) ? h->partC.d() : h->partB.d();
    bool on = false;
    if (h->pr_packed) SRCCHK2(h, {f.pr.q_old, 2}, {f.pr.px_old, 2});
    else SRCCHK2(h, {f.pr.z_old, 1}, {f.pr.zs_old, 1}, {f.pr.p_old, 1});
    prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
    const int grid = launch_win_pr_one(h->sc, h->wdev(), h->wtile_ptr(0), h->nwt_int + h->nwt_bnd, h->win_geom, f,
                                       (meurant(h->variant) ? 1 : 0) | (h->stream_stores ? 2 : 0), part_out, coef_at(h, k), h->opt.win_per_cu);
    LAUNCHCHK(h, grid);
    prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
    h->pend_parts = grid; h->pend_k = k; h->pend_buf = part_out;
    note_partials_launch(h, grid);
    if (h->pr_packed) h->q_cur = f.pr.q_new;
    else { z_cur = z_new; zs_cur = zs_new; h->p_cur = p_new; }
    return PRCG_OK;
}

// end of a prcg_iterate call of a packed predict-and-recompute session: the packed entries back into r, s, p, x
void pr_unpack(prcg_t* h) {
    if (!h->pr_packed || !h->pr_q_valid) return;
    const size_t half = (size_t)2 * (h->n + h->g + kGatherPad);
    launch_copy(h->sc, h->cur_r, 1, h->q_cur + 0, 2, h->n);
    launch_copy(h->sc, h->cur_s, 1, h->q_cur + 1, 2, h->n);
    launch_copy(h->sc, h->p_cur, 1, h->q_cur + half + 0, 2, h->n);
    launch_copy(h->sc, h->x.d(), 1, h->q_cur + half + 1, 2, h->n);
    h->pr_q_valid = false;
}

PrArgs pr_args(prcg_t* h, int k) {
    PrArgs a{};
    a.n = h->n;
    a.x = h->x.d(); a.r = h->r.d(); a.rt = h->prec ? h->rt.d() : nullptr;
    a.p = h->p.d(); a.s = h->s.d(); a.st_ = h->prec ? h->st.d() : nullptr;
    a.dots_prev = k > 0 ? dots_at(h, k - 1) : dots_at(h, 0);
    a.coef_out = coef_at(h, k);
    a.partials = h->partA.d();
    a.meurant = meurant(h->variant);
    a.precond = h->prec;
    return a;
}

int pr_spmv_and_reduce(prcg_t* h, int k, int grid_upd) {
    // s = A p; s~ = M^-1 s; mu, delta, gamma ride on the SpMV (pr_cg.py:152-157)
    int nparts = 0;
    int rc;
    if (h->stored_tilde) {
        // s = A p; s~ = preconditioner(s) (host callback or block-Jacobi launch); mu, delta, gamma as inner products of their own
        if ((rc = overlapped_spmv(h, k, h->p.d(), h->s.d(), kEpiNone, nullptr, nullptr, nullptr, &nparts))) return rc;
        if ((rc = apply_prec(h, h->s.d(), 1, h->st.d(), 1))) return rc;
        int g = launch_dot(h->sc, h->p.d(), h->s.d(), h->n, h->partB.d(), 0);
        LAUNCHCHK(h, g);
        LAUNCHCHK(h, launch_dot(h->sc, h->r.d(), h->st.d(), h->n, h->partB.d(), 1));
        LAUNCHCHK(h, launch_dot(h->sc, h->st.d(), h->s.d(), h->n, h->partB.d(), 2));
        launch_reduce_final(h->sc, h->partA.d(), grid_upd, dots_at(h, k), PRCG_S_NU, PRCG_S_NU, 2);
        launch_reduce_final(h->sc, h->partB.d(), g, dots_at(h, k), 0, 0, 3);
        return allreduce(h, dots_at(h, k), 5, h->sc);
    }
    rc = overlapped_spmv(h, k, h->p.d(), h->s.d(), kEpiPR, h->r.d(), h->prec ? h->dinv.d() : nullptr,
                         h->prec ? h->st.d() : nullptr, &nparts);
    if (rc) return rc;
    launch_reduce_final(h->sc, h->partA.d(), grid_upd, dots_at(h, k), PRCG_S_NU, PRCG_S_NU, 2);
    launch_reduce_final(h->sc, h->partB.d(), nparts, dots_at(h, k), 0, 0, 3);
    return allreduce(h, dots_at(h, k), 5, h->sc);                       // the one reduction
}

int iterate_pr(prcg_t* h, int k) {
    PrArgs a = pr_args(h, k);
    bool on = false;
    prof_begin(h, h->ev_upd, h->n_ev_upd, k, on);
    const int grid = launch_pr_update(h->sc, a);
    LAUNCHCHK(h, grid);
    prof_end(h, h->ev_upd, h->n_ev_upd, on);
    return pr_spmv_and_reduce(h, k, grid);
}

CgArgs cg_args(prcg_t* h, int k) {
    CgArgs a{};
    a.n = h->n;
    a.x = h->x.d(); a.r = h->cur_r; a.rt = h->prec ? h->rt.d() : nullptr;
    a.w = h->cur_w; a.wt = h->prec ? h->wt.d() : nullptr;
    a.p = h->p.d(); a.s = h->cur_s;
    a.st_ = (h->prec && h->variant == PRCG_GV) ? h->st.d() : nullptr;
    a.u = h->variant == PRCG_GV ? h->cur_u : nullptr;
    a.t = h->cur_t;
    a.z = h->prec ? h->rt.d() : h->cur_r;
    a.d = (h->prec && !h->stored_tilde) ? h->dinv.d() : nullptr;
    a.dots_prev = k > 0 ? dots_at(h, k - 1) : dots_at(h, 0);
    a.dots_cur = dots_at(h, k);
    a.dots_cur_w = dots_at(h, k);
    a.coef_out = coef_at(h, k);
    a.partials = h->partA.d();
    return a;
}

// Chronopoulos-Gear on a window operator in TWO launches (was four): the product launch forms its window as the new
// residual r - a s (times d), writes x, r, r~, w and the partials of eta, nu; the p, s update sums them in its prologue
// (same tree as k_reduce_final), derives b and mu and leaves the complete scalars of iteration k behind.
int iterate_cgcg_fused(prcg_t* h, int k) {
    double* r_new = (h->cur_r == h->r.d()) ? h->r2.d() : h->r.d();
    FusedPrev f{};
    f.dots_old = dots_at(h, k - 1);
    f.pr.z_old = h->cur_r; f.pr.zs_old = h->s.d(); f.pr.p_old = h->p.d();
    f.pr.z_new = r_new; f.pr.zs_new = h->prec ? h->rt.d() : nullptr;
    f.pr.x = h->x.d(); f.pr.d = h->prec ? h->dinv.d() : nullptr;
    bool on = false;
    SRCCHK2(h, {f.pr.z_old, 1}, {f.pr.zs_old, 1}, {f.pr.d, 1});
    prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
    const int grid = launch_win_cg_w(h->sc, h->wdev(), h->wtile_ptr(0), h->nwt_int + h->nwt_bnd, h->win_geom, f, h->w.d(),
                                     h->partB.d(), coef_at(h, k), h->opt.win_per_cu);
    LAUNCHCHK(h, grid);
    note_partials_launch(h, grid);
    prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
    h->cur_r = r_new;
    on = false;
    prof_begin(h, h->ev_upd, h->n_ev_upd, k, on);
    LAUNCHCHK(h, launch_cg_update_ps(h->sc, cg_args(h, k), h->partB.d(), grid));
    prof_end(h, h->ev_upd, h->n_ev_upd, on);
    return PRCG_OK;
}

// Ghysels-Vanroose in two launches, the same way: the window is the new w formed as w - a u (times d).
int iterate_gv_fused(prcg_t* h, int k) {
    double* w_new = (h->cur_w == h->w.d()) ? h->w2.d() : h->w.d();
    FusedPrev f{};
    f.dots_old = dots_at(h, k - 1);
    f.pr.z_old = h->cur_w; f.pr.zs_old = h->u.d(); f.pr.p_old = h->p.d();
    f.pr.z_new = w_new; f.pr.zs_new = h->prec ? h->wt.d() : nullptr;
    f.pr.x = h->x.d(); f.pr.r = h->r.d(); f.pr.s = h->s.d();
    f.pr.d = h->prec ? h->dinv.d() : nullptr;
    f.pr.rt = h->prec ? h->rt.d() : nullptr; f.pr.st = h->prec ? h->st.d() : nullptr;
    bool on = false;
    SRCCHK2(h, {f.pr.z_old, 1}, {f.pr.zs_old, 1}, {f.pr.d, 1});
    prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
    const int grid = launch_win_gv_w(h->sc, h->wdev(), h->wtile_ptr(0), h->nwt_int + h->nwt_bnd, h->win_geom, f, h->tvec.d(),
                                     h->partB.d(), coef_at(h, k), h->opt.win_per_cu);
    LAUNCHCHK(h, grid);
    note_partials_launch(h, grid);
    prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
    h->cur_w = w_new;
    on = false;
    prof_begin(h, h->ev_upd, h->n_ev_upd, k, on);
    LAUNCHCHK(h, launch_cg_update_ps(h->sc, cg_args(h, k), h->partB.d(), grid));
    prof_end(h, h->ev_upd, h->n_ev_upd, on);
    return PRCG_OK;
}

// close the iteration whose p, s (u) update is still pending (one-launch Chronopoulos-Gear / Ghysels-Vanroose): what the
// next launch would do while forming its window, as a launch of its own -- at the end of a prcg_iterate call, before a recorder
void cg_flush(prcg_t* h) {
    if (!h->cg_lag) return;
    if (h->prec) launch_mul(h->sc, h->rt.d(), 1, h->dinv.d(), 1, h->cur_r, 1, h->n);        // r~ = M^-1 r (the launches keep it in registers)
    (void)launch_cg_update_ps(h->sc, cg_args(h, h->pend_k), h->pend_buf, h->pend_parts);
    h->cg_lag = false;
    h->pend_parts = 0;
}

// Finish what the last launch of the session left pending, each schedule its own: inner products that exist only as block
// partials, the packed state, the deferred p, s update, the communication chain of the last iteration.  Called before a
// recorder runs (it reuses the partials buffers and reads the state vectors) and at the end of prcg_iterate (the caller
// may read or rewrite state next: recorders, teacher forcing).
int flush_pending(prcg_t* h) {
    Session& s = *h;
    if (s.fused && !s.fused_comm) fused_flush(h);
    if (s.hs_fused) hs_flush(h);
    if (s.pr_fused) { fused_flush(h); pr_unpack(h); }
    if (s.cg_one) cg_flush(h);
    if (s.fused_comm && s.red_pending) HIPCHK(h, hipStreamWaitEvent(h->sc, s.red_event, 0));
    if (s.peer && s.pend_parts > 0) {
        // peer exchange: the last launch's partials are sent by the NEXT launch's communication wave -- there may be none, or
        // a recorder is about to reuse the buffer: this rank's slot goes out now, then every rank's slot is added in rank order
        launch_peer_collect(h->sc, static_cast<const PeerDev*>(h->peer_dev.p), s.pend_k, s.pend_buf, s.pend_parts, dots_at(h, s.pend_k),
                            h->pub.d(), static_cast<unsigned*>(h->pub_err.p));
        s.pend_parts = 0;
    }
    return PRCG_OK;
}

// ONE launch per iteration of Chronopoulos-Gear / Ghysels-Vanroose on a window operator (launch_win_cg_one): the launch of
// iteration k closes iteration k-1 in its prologue (b, mu, a from that launch's partials) and applies its p, s (u) update
// while forming the window -- the new residual (new w) expressed in old vectors.
int iterate_cg_one(prcg_t* h, int k) {
    const bool gv = h->variant == PRCG_GV;
    if (h->cg_lag && h->pend_k != k - 1) cg_flush(h);
    FusedPrev f{};
    if (h->cg_lag) {
        f.prev_partials = h->pend_buf; f.nprev = h->pend_parts;
        f.dots_prev_out = dots_at(h, k - 1); f.dots_old = dots_at(h, k - 2); f.lag.coef_prev = coef_at(h, k - 1);
    } else {
        f.dots_old = dots_at(h, k - 1);
    }
    auto other = [](double* cur, DevBuf& a, DevBuf& b) { return cur == a.d() ? b.d() : a.d(); };
    double *z0n, *z1n, *z2n;
    if (gv) {
        f.lag.z0 = h->cur_w; f.lag.z1 = h->cur_t; f.lag.z2 = h->cur_u;
        z0n = other(h->cur_w, h->w, h->w2); z1n = other(h->cur_t, h->tvec, h->t2); z2n = other(h->cur_u, h->u, h->u2);
        f.lag.r = h->r.d(); f.lag.s = h->s.d();
    } else {
        f.lag.z0 = h->cur_r; f.lag.z1 = h->cur_w; f.lag.z2 = h->cur_s;
        z0n = other(h->cur_r, h->r, h->r2); z1n = other(h->cur_w, h->w, h->w2); z2n = other(h->cur_s, h->s, h->s2);
        f.lag.d = h->prec ? h->dinv.d() : nullptr;
    }
    f.lag.z0n = z0n; f.lag.z1n = z1n; f.lag.z2n = z2n;
    f.lag.x = h->x.d(); f.lag.p = h->p.d();
    double* part_out = (h->pend_buf == h->partB.d()) ? h->partC.d() : h->partB.d();
    SRCCHK2(h, {f.lag.z0, 1}, {f.lag.z1, 1}, {f.lag.z2, 1}, {f.lag.d, 1});
    bool on = false;
    prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
    const int grid = launch_win_cg_one(h->sc, h->wdev(), h->wtile_ptr(0), h->nwt_int + h->nwt_bnd, h->win_geom, f, gv ? 1 : 0, part_out,
                                       coef_at(h, k), h->opt.win_per_cu);
    LAUNCHCHK(h, grid);
    note_partials_launch(h, grid);
    prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
    if (gv) { h->cur_w = z0n; h->cur_t = z1n; h->cur_u = z2n; }
    else { h->cur_r = z0n; h->cur_w = z1n; h->cur_s = z2n; }
    h->pend_parts = grid; h->pend_k = k; h->pend_buf = part_out; h->cg_lag = true;
    return PRCG_OK;
}

// Chronopoulos-Gear (cg_cg.py:59-68): ONE reduction per iteration, after the SpMV it depends on
int iterate_cgcg(prcg_t* h, int k) {
    HsArgs a = hs_args(h, k);
    bool on = false;
    prof_begin(h, h->ev_upd, h->n_ev_upd, k, on);
    LAUNCHCHK(h, launch_hs_update_xr(h->sc, a));                              // x, r, (r~)
    prof_end(h, h->ev_upd, h->n_ev_upd, on);
    double* z = h->prec ? h->rt.d() : h->r.d();
    int nparts = 0;
    int rc;
    if (h->stored_tilde && (rc = apply_prec(h, h->r.d(), 1, h->rt.d(), 1))) return rc;   // r~ = preconditioner(r)  cg_cg.py:118
    rc = overlapped_spmv(h, k, z, h->w.d(), kEpiCG, h->r.d(), nullptr, nullptr, &nparts);   // w = A r~; nu, eta
    if (rc) return rc;
    launch_reduce_final(h->sc, h->partB.d(), nparts, dots_at(h, k), 0, 0, 5);
    if ((rc = allreduce(h, dots_at(h, k), 5, h->sc))) return rc;
    LAUNCHCHK(h, launch_cg_update_ps(h->sc, cg_args(h, k)));                  // p, s; mu by recurrence
    return PRCG_OK;
}

// Ghysels-Vanroose (gv_cg.py:65-81): the inner products come BEFORE the SpMV they overlap with
int iterate_gv(prcg_t* h, int k) {
    CgArgs a = cg_args(h, k);
    bool on = false;
    prof_begin(h, h->ev_upd, h->n_ev_upd, k, on);
    const int grid = launch_gv_update1(h->sc, a, false);                      // x, r, r~, w, w~; nu, eta
    LAUNCHCHK(h, grid);
    prof_end(h, h->ev_upd, h->n_ev_upd, on);
    int rc;
    bool replaced = false;
    if (h->replace_fn) {
        // gv_cg.py:69-71: the caller's predicate sees the state as the reference passes it (x, r, w new; p, s, u old)
        HIPCHK(h, hipStreamSynchronize(h->sc));
        const int kk = h->k;
        h->k = k;                                                        // (prcg_get_* inside the hook address iteration k)
        const int fire = h->replace_fn(h->replace_ctx, k);
        h->k = kk;
        if (fire) {
            if ((rc = dist_spmv(h, h->r.d(), h->cur_w, kEpiNone, nullptr, nullptr, nullptr, nullptr))) return rc;   // w = A r
            if (h->prec && !h->stored_tilde) launch_mul(h->sc, h->wt.d(), 1, h->dinv.d(), 1, h->cur_w, 1, h->n);      // w~ = M^-1 w
            replaced = true;
        }
    }
    if (h->stored_tilde && (rc = apply_prec(h, h->w.d(), 1, h->wt.d(), 1))) return rc;  // w~ = preconditioner(w)  gv_cg.py:161
    const bool side = h->multi() && !h->replace_fn;
    if (side) {
        HIPCHK(h, hipEventRecord(h->e_upd, h->sc));
        HIPCHK(h, hipStreamWaitEvent(h->sm, h->e_upd, 0));
        launch_reduce_final(h->sm, h->partA.d(), grid, dots_at(h, k), 0, 0, 5);
        if ((rc = allreduce(h, dots_at(h, k), 5, h->sm))) return rc;
        HIPCHK(h, hipEventRecord(h->e_red, h->sm));
    } else {
        launch_reduce_final(h->sc, h->partA.d(), grid, dots_at(h, k), 0, 0, 5);
        if (replaced) {     // eta = w.r~ with the replaced w (gv_cg.py:75 / :164)
            const int g2 = launch_dot(h->sc, h->cur_w, h->prec ? h->rt.d() : h->r.d(), h->n, h->partB.d(), 0);
            LAUNCHCHK(h, g2);
            launch_reduce_final(h->sc, h->partB.d(), g2, dots_at(h, k), 0, PRCG_S_DELTA, 1);
        }
        if (h->multi() && (rc = allreduce(h, dots_at(h, k), 5, h->sc))) return rc;
    }
    double* zt = h->prec ? h->wt.d() : h->w.d();
    int nparts = 0;
    if ((rc = overlapped_spmv(h, k, zt, h->tvec.d(), kEpiNone, nullptr, nullptr, nullptr, &nparts))) return rc;   // t = A w~
    if (side) HIPCHK(h, hipStreamWaitEvent(h->sc, h->e_red, 0));
    LAUNCHCHK(h, launch_cg_update_ps(h->sc, a));                              // p, s, s~, u; mu by recurrence
    return PRCG_OK;
}

int h2d(prcg_t* h, double* dst, const double* src, int64_t count) {
    HIPCHK(h, hipMemcpyAsync(dst, src, (size_t)count * sizeof(double), hipMemcpyHostToDevice, h->sc));
    HIPCHK(h, hipStreamSynchronize(h->sc));
    return PRCG_OK;
}
int d2h(prcg_t* h, double* dst, const double* src, int64_t count) {
    HIPCHK(h, hipMemcpyAsync(dst, src, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, h->sc));
    HIPCHK(h, hipStreamSynchronize(h->sc));
    return PRCG_OK;
}

// dst = M^-1 src: the inverse diagonal or the inverse diagonal blocks on the device, or the caller's function on the
// host (the reference's `preconditioner(v)`, figure_gen.py:42-44 -- there, too, it is the caller's Python callable).
int apply_prec(prcg_t* h, const double* src, int sstride, double* dst, int dstride) {
    const int64_t n = h->n;
    if (!h->stored_tilde) {
        launch_mul(h->sc, dst, dstride, h->dinv.d(), 1, src, sstride, n);
        return PRCG_OK;
    }
    if (h->bj_session) {        // one launch on the compute stream: no copy, no synchronisation
        if (h->bj_var)
            LAUNCHCHK(h, launch_block_jacobi_var(h->sc, dst, dstride, src, sstride, h->bjv_plan.ntiles, h->bjv_tiles_d(), h->bjv_code_d(), h->bj_blocks.d()));
        else
            LAUNCHCHK(h, launch_block_jacobi(h->sc, dst, dstride, src, sstride, n, h->bj_bs, h->bj_blocks.d()));
        return PRCG_OK;
    }
    h->cb_in.resize((size_t)n); h->cb_out.resize((size_t)n);
    const double* dsrc = src;
    if (sstride != 1) { launch_copy(h->sc, h->cb_stage.d(), 1, src, sstride, n); dsrc = h->cb_stage.d(); }
    int rc = d2h(h, h->cb_in.data(), dsrc, n);
    if (rc) return rc;
    if (h->cb(h->cb_ctx, n, h->cb_in.data(), h->cb_out.data()) != 0)
        return fail(h, PRCG_EINVAL, "the preconditioner callback reported a failure");
    if (dstride == 1) return h2d(h, dst, h->cb_out.data(), n);
    if ((rc = h2d(h, h->cb_stage.d(), h->cb_out.data(), n))) return rc;
    launch_copy(h->sc, dst, dstride, h->cb_stage.d(), 1, n);
    return PRCG_OK;
}

// where does state vector `which` live?  base pointer + stride (in doubles)
bool locate(prcg_t* h, int which, double** base, int* stride) {
    *stride = 1;
    *base = nullptr;
    const int v = h->variant;
    if (is_pipe(v)) {
        switch (which) {
        case PRCG_VEC_X: *base = h->xp.d(); *stride = 2; return true;
        case PRCG_VEC_P: *base = h->xp.d() + 1; *stride = 2; return true;
        case PRCG_VEC_R: *base = ((h->fused && !h->prec) ? h->rs_cur : h->rs.d()); *stride = 2; return true;
        case PRCG_VEC_S: *base = ((h->fused && !h->prec) ? h->rs_cur : h->rs.d()) + 1; *stride = 2; return true;
        case PRCG_VEC_W:
            if (h->fused) { if (pipe_recompute(v)) return false; *base = h->wv.d(); return true; }   // stored recurrence
            *base = h->wu.d(); *stride = 2; return true;
        case PRCG_VEC_U: if (h->fused) return false; *base = h->wu.d() + 1; *stride = 2; return true;
        case PRCG_VEC_RT: if (!h->prec) return false; *base = (h->fused ? h->rs_cur : h->rst.d()); *stride = 2; return true;
        case PRCG_VEC_ST: if (!h->prec) return false; *base = (h->fused ? h->rs_cur : h->rst.d()) + 1; *stride = 2; return true;
        // stored-tilde sessions (host callback, block Jacobi): w~ and u~ are stored state (what M^-1 returned), in every flavour
        case PRCG_VEC_WT: if (!h->prec || (pipe_recompute(v) && !h->stored_tilde)) return false; *base = h->wt.d(); return true;
        case PRCG_VEC_UT: if (!h->stored_tilde) return false; *base = h->ut.d(); return true;
        default: return false;
        }
    }
    if (is_cg_family(v)) {
        switch (which) {
        case PRCG_VEC_X: *base = h->x.d(); return true;
        case PRCG_VEC_P: *base = h->p.d(); return true;
        case PRCG_VEC_R: *base = h->cur_r; return true;
        case PRCG_VEC_S: *base = h->cur_s; return true;
        case PRCG_VEC_W: *base = h->cur_w; return true;
        case PRCG_VEC_U: if (v != PRCG_GV) return false; *base = h->cur_u; return true;
        case PRCG_VEC_RT: if (!h->prec) return false; *base = h->rt.d(); return true;
        case PRCG_VEC_WT: if (!h->prec || v != PRCG_GV) return false; *base = h->wt.d(); return true;
        case PRCG_VEC_ST: if (!h->prec || v != PRCG_GV) return false; *base = h->st.d(); return true;
        default: return false;
        }
    }
    switch (which) {
    case PRCG_VEC_X: *base = h->x.d(); return true;
    case PRCG_VEC_P: *base = h->p_cur; return true;
    case PRCG_VEC_R: *base = h->cur_r; return true;
    case PRCG_VEC_S: *base = h->cur_s; return true;
    case PRCG_VEC_RT: if (!h->prec) return false; *base = h->cur_rt; return true;
    case PRCG_VEC_ST: if (!h->prec || !is_pr(v)) return false; *base = h->cur_st; return true;
    default: return false;
    }
}

// forget the block-Jacobi blocks; a session that applies them ends here (its launches may still be reading them: wait)
int drop_block_jacobi(prcg_t* h) {
    if (!h->have_block_jacobi() && !h->bj_blocks.p) return PRCG_OK;
    HIPCHK(h, hipSetDevice(h->dev));
    HIPCHK(h, hipStreamSynchronize(h->sc));
    if (h->bj_session) { h->in_session = false; h->bj_session = false; }
    h->bj_bs = 0;
    h->bj_blocks.release();
    h->bj_var = false;                   // the variable kind: its tables go with its blocks
    h->bjv_tiles.release(); h->bjv_bytes.release();
    h->bjv_plan = BjVarPlan{}; h->bjv_ptr.clear();
    return PRCG_OK;
}

template <typename T>
int upload(prcg_t* h, DevBuf& dst, const std::vector<T>& src) {
    if (!src.empty()) HIPCHK(h, hipMemcpy(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return PRCG_OK;
}

// the arrays of a plan into the handle's device buffers (padded so the 16-byte stream loads never leave the allocation)
int upload_operator(prcg_t* h, const OperatorPlan& pl, const int32_t* ip, const int32_t* indices, const double* data) {
    Operator& op = *h;
    const int64_t n_rows = pl.n, nnz = pl.nnz;
    const size_t pad = 32;
    int rc;
    HIPCHK(h, op.indptr.alloc(((size_t)n_rows + 1 + pad) * sizeof(int32_t)));
    HIPCHK(h, op.col.alloc(((size_t)nnz + pad) * sizeof(int32_t)));
    HIPCHK(h, op.val.alloc(((size_t)nnz + pad) * sizeof(double)));
    HIPCHK(h, op.tiles.alloc((pl.tiles.size() + 1) * sizeof(Tile)));
    HIPCHK(h, hipMemcpy(op.indptr.p, ip, ((size_t)n_rows + 1) * sizeof(int32_t), hipMemcpyHostToDevice));
    if (nnz > 0) {
        HIPCHK(h, hipMemcpy(op.col.p, indices, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(h, hipMemcpy(op.val.p, data, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
    }
    if ((rc = upload(h, op.tiles, pl.tiles))) return rc;
    HIPCHK(h, op.tile_base.alloc(pl.tbase.size() * sizeof(int32_t)));
    if ((rc = upload(h, op.tile_base, pl.tbase))) return rc;
    HIPCHK(h, op.col16.alloc(pl.c16.empty() ? 16 : pl.c16.size() * sizeof(uint16_t)));
    if ((rc = upload(h, op.col16, pl.c16))) return rc;
    HIPCHK(h, op.col8.alloc(pl.c8.empty() ? 16 : pl.c8.size()));
    if ((rc = upload(h, op.col8, pl.c8))) return rc;
    const bool any_vd = pl.vd_int || pl.vd_bnd;
    HIPCHK(h, op.vidx8.alloc(any_vd ? pl.vidx.size() : 16));
    HIPCHK(h, op.vdict.alloc(any_vd ? (pl.vdict.size() + kDictMax) * sizeof(double) : 16));
    HIPCHK(h, op.vdesc.alloc(any_vd ? pl.vdesc.size() * sizeof(int32_t) : 16));
    if (any_vd) {
        if ((rc = upload(h, op.vidx8, pl.vidx))) return rc;
        if ((rc = upload(h, op.vdict, pl.vdict))) return rc;
        if ((rc = upload(h, op.vdesc, pl.vdesc))) return rc;
    }
    if (pl.sell) {
        const SellPlan& sp = pl.sp;
        HIPCHK(h, op.sval.alloc(sp.val.size() * sizeof(double), false));
        if ((rc = upload(h, op.sval, sp.val))) return rc;
        HIPCHK(h, op.scol.alloc(sp.col.size() * sizeof(uint16_t), false));
        if ((rc = upload(h, op.scol, sp.col))) return rc;
        HIPCHK(h, op.sslices.alloc((pl.sslices.size() + 1) * sizeof(SellSlice)));
        if ((rc = upload(h, op.sslices, pl.sslices))) return rc;
        HIPCHK(h, op.srows.alloc((sp.rows.size() + 64) * sizeof(int32_t)));
        if ((rc = upload(h, op.srows, sp.rows))) return rc;
        HIPCHK(h, op.sgran.alloc((sp.gran.size() + 64) * sizeof(int32_t)));
        if ((rc = upload(h, op.sgran, sp.gran))) return rc;
    }
    if (pl.win) {
        if (pl.win_pat) {
            // pattern tiles: the rows' slot masks (wrel) take the place of the row pointers; no window-index images
            HIPCHK(h, op.wcw.alloc(64));
            HIPCHK(h, op.wpat.alloc((pl.pats.size() + 1) * sizeof(PatRec)));
            if ((rc = upload(h, op.wpat, pl.pats))) return rc;
        } else if (pl.win_geom >= 2) {
            HIPCHK(h, op.wcw.alloc(pl.wcw16.size() * sizeof(uint16_t)));
            if ((rc = upload(h, op.wcw, pl.wcw16))) return rc;
        } else {
            HIPCHK(h, op.wcw.alloc(pl.wcw8.size()));
            if ((rc = upload(h, op.wcw, pl.wcw8))) return rc;
        }
        HIPCHK(h, op.wrel.alloc(pl.wrel.size() * sizeof(uint16_t)));
        if ((rc = upload(h, op.wrel, pl.wrel))) return rc;
        HIPCHK(h, op.wtiles.alloc((pl.wtiles.size() + 1) * sizeof(WTile)));
        if ((rc = upload(h, op.wtiles, pl.wtiles))) return rc;
        if (pl.win_vd) {
            HIPCHK(h, op.wvidx.alloc(pl.wvidx.size()));
            if ((rc = upload(h, op.wvidx, pl.wvidx))) return rc;
            HIPCHK(h, op.wvdict.alloc((pl.wvdict.size() + kWinDictMax) * sizeof(double)));
            if ((rc = upload(h, op.wvdict, pl.wvdict))) return rc;
        }
    }
    HIPCHK(h, h->tmp_ext.alloc((size_t)2 * (n_rows + pl.g + kGatherPad) * sizeof(double)));
    HIPCHK(h, h->t1.alloc((size_t)2 * n_rows * sizeof(double)));
    HIPCHK(h, h->partA.alloc((size_t)8192 * kPartialStride * sizeof(double)));
    HIPCHK(h, h->partB.alloc((size_t)8192 * kPartialStride * sizeof(double)));
    return PRCG_OK;
}

// 32-bit row pointers, checked: inside [0, nnz], monotone, from 0 to nnz
int checked_indptr(prcg_t* h, int64_t n_rows, int64_t nnz, const void* indptr, int indptr_is64, std::vector<int32_t>& ip) {
    ip.resize((size_t)n_rows + 1);
    for (int64_t i = 0; i <= n_rows; ++i) {
        const int64_t v = indptr_is64 ? static_cast<const int64_t*>(indptr)[i] : static_cast<const int32_t*>(indptr)[i];
        CHECK(h, v >= 0 && v <= nnz, "prcg_set_csr: indptr[%lld]=%lld out of [0,nnz]", (long long)i, (long long)v);
        CHECK(h, i == 0 || v >= ip[i - 1], "prcg_set_csr: indptr not monotone at row %lld", (long long)i);
        ip[i] = (int32_t)v;
    }
    CHECK(h, ip[0] == 0 && ip[n_rows] == nnz, "prcg_set_csr: indptr must run from 0 to nnz");
    return PRCG_OK;
}

// plan_operator (host only, prcg_plan.cpp) -> upload the plan's arrays -> keep its flags: what prcg_set_csr does with validated
// arrays, and what the re-planning route of prcg_update_values does with the arrays it read back
int install_operator(prcg_t* h, int64_t n_rows, int64_t n_ghost, int64_t nnz, const int32_t* ip, const int32_t* indices, const double* data) {
    OperatorPlan pl;
    std::string why;
    if (!plan_operator(h->opt, n_rows, n_ghost, nnz, ip, indices, data, pl, why)) return fail(h, PRCG_EINVAL, "%s", why.c_str());
    // (the flags describe the upload in progress, as they always have: a failed upload leaves have_csr as it was)
    static_cast<OperatorShape&>(*h) = pl;
    if (int rc = upload_operator(h, pl, ip, indices, data)) return rc;
    h->peer_ok = false;
    h->wt_rb.clear(); h->wt_re.clear();
    if (pl.win)
        for (const WTile& t : pl.wtiles) { h->wt_rb.push_back(t.rb); h->wt_re.push_back(t.re); }
    h->have_csr = true;
    return PRCG_OK;
}

// A caller's device pointer is read only after the runtime has vouched for it: device memory of the handle's GPU, and
// [p, p + bytes) inside the allocation it belongs to
int checked_device_range(prcg_t* h, const char* who, const void* p, size_t bytes) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, PRCG_EINVAL, "%s: data_on_device = 1, but the runtime knows no allocation at %p", who, p);
    }
    CHECK(h, at.type == hipMemoryTypeDevice, "%s: data_on_device = 1, but %p is not device memory (memory type %d)", who, p, (int)at.type);
    CHECK(h, at.device == h->dev, "%s: the values lie on GPU %d, the handle's GPU is %d", who, at.device, h->dev);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void*>(p)) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, PRCG_EINVAL, "%s: no address range for the device pointer %p", who, p);
    }
    const char* lo = static_cast<const char*>(base);
    const char* c = static_cast<const char*>(p);
    CHECK(h, c >= lo && bytes <= size && (size_t)(c - lo) <= size - bytes,
          "%s: %zu bytes from %p leave the allocation they begin in (%zu bytes from %p)", who, bytes, p, size, (void*)base);
    return PRCG_OK;
}

uint64_t fnv1a(uint64_t hash, const void* data, size_t bytes) {
    const unsigned char* c = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < bytes; ++i) { hash ^= c[i]; hash *= 0x100000001b3ull; }
    return hash;
}
template <typename T>
uint64_t fnv1a(uint64_t hash, const std::vector<T>& v) { return fnv1a(hash, v.data(), v.size() * sizeof(T)); }

void destroy_events(std::vector<EventPair>& evs) {
    for (auto& e : evs) { if (e.a) (void)hipEventDestroy(e.a); if (e.b) (void)hipEventDestroy(e.b); }
    evs.clear();
}

}  // namespace

// =========================================================================================
extern "C" {

int prcg_version(void) { return 1; }

const char* prcg_last_error(const prcg_t* h) { return h ? h->err.c_str() : g_last_error.c_str(); }

int prcg_create(prcg_t** out, int device_id) {
    if (!out) return fail(nullptr, PRCG_EINVAL, "prcg_create: null output pointer");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(nullptr, PRCG_EHIP, "prcg_create: no HIP device available (%s); this library has no CPU fallback",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= ndev)
        return fail(nullptr, PRCG_EINVAL, "prcg_create: device %d out of range [0,%d)", device_id, ndev);
    e = hipSetDevice(device_id);
    if (e != hipSuccess) return fail(nullptr, PRCG_EHIP, "hipSetDevice(%d): %s", device_id, hipGetErrorString(e));
    prcg_t* h = new (std::nothrow) prcg_handle();
    if (!h) return fail(nullptr, PRCG_ENOMEM, "out of host memory");
    h->dev = device_id;
    // every switch lives in the handle from here on (no lazily read environment anywhere else)
    for (int i = 0; i < kNumOptions; ++i)
        if (const char* e = getenv(kOptions[i].key)) kOptions[i].set(h->opt, atol(e));
    // the communication stream outranks the compute stream: its small kernels (halo pack,
    // partial reduction, RCCL) must get CU slots while the matrix product floods the chip
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    if (hipStreamCreateWithPriority(&h->sc, hipStreamNonBlocking, prio_lo) != hipSuccess ||
        hipStreamCreateWithPriority(&h->sm, hipStreamNonBlocking, prio_hi) != hipSuccess ||
        hipStreamCreateWithPriority(&h->sh, hipStreamNonBlocking, prio_hi) != hipSuccess ||
        hipEventCreateWithFlags(&h->e_upd, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->e_halo, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->e_red, hipEventDisableTiming) != hipSuccess ||
        hipEventCreate(&h->e_kdone) != hipSuccess || hipEventCreate(&h->e_rdone) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void**>(&h->err_host), 64, hipHostMallocDefault) != hipSuccess) {
        prcg_destroy(h);
        return fail(nullptr, PRCG_EHIP, "prcg_create: stream/event creation failed");
    }
    *h->err_host = 0u;
    *out = h;
    return PRCG_OK;
}

void prcg_destroy(prcg_t* h) {
    if (!h) return;
    (void)hipSetDevice(h->dev);
    (void)hipDeviceSynchronize();
    for (void* q : h->peer_opened) (void)hipIpcCloseMemHandle(q);
    if (h->xbuf) (void)hipFree(h->xbuf);
    if (h->err_host) (void)hipHostFree(h->err_host);
    if (h->comm_halo && h->rccl) (void)h->rccl->CommDestroy(h->comm_halo);
    if (h->comm && h->rccl) (void)h->rccl->CommDestroy(h->comm);
    destroy_events(h->ev_spmv);
    destroy_events(h->ev_upd);
    if (h->e_upd) (void)hipEventDestroy(h->e_upd);
    if (h->e_halo) (void)hipEventDestroy(h->e_halo);
    if (h->e_red) (void)hipEventDestroy(h->e_red);
    if (h->e_kdone) (void)hipEventDestroy(h->e_kdone);
    if (h->e_rdone) (void)hipEventDestroy(h->e_rdone);
    if (h->sc) (void)hipStreamDestroy(h->sc);
    if (h->sm) (void)hipStreamDestroy(h->sm);
    if (h->sh) (void)hipStreamDestroy(h->sh);
    delete h;
}

int prcg_set_preconditioner(prcg_t* h, prcg_prec_fn fn, void* ctx) {
    if (!h) return PRCG_EINVAL;
    h->cb = fn;
    h->cb_ctx = ctx;
    if (fn) return drop_block_jacobi(h);         // the last preconditioner set is the one in force
    return PRCG_OK;
}

int prcg_set_block_jacobi(prcg_t* h, int bs, const double* inv_blocks) {
    if (!h) return PRCG_EINVAL;
    if (!inv_blocks) return drop_block_jacobi(h);
    CHECK(h, bs >= 1 && bs <= 8, "prcg_set_block_jacobi: block size %d outside 1..8", bs);
    CHECK(h, h->have_csr, "prcg_set_block_jacobi: call prcg_set_csr first (the blocks are sized by its n_rows)");
    CHECK(h, !h->multi(), "a block-Jacobi preconditioner runs on one GPU only");
    if (int rc = drop_block_jacobi(h)) return rc;
    const int64_t count = block_jacobi_layout(h->n, bs, inv_blocks, nullptr);
    std::vector<double> laid;
    try { laid.resize((size_t)count); } catch (const std::bad_alloc&) { return fail(h, PRCG_ENOMEM, "out of host memory"); }
    block_jacobi_layout(h->n, bs, inv_blocks, laid.data());
    HIPCHK(h, h->bj_blocks.alloc((size_t)count * sizeof(double), false));
    HIPCHK(h, hipMemcpy(h->bj_blocks.p, laid.data(), (size_t)count * sizeof(double), hipMemcpyHostToDevice));
    h->bj_bs = bs;
    h->cb = nullptr; h->cb_ctx = nullptr;        // the last preconditioner set is the one in force
    return PRCG_OK;
}

// The blocks from the operator itself: one launch over the caller-order CSR arrays upload_operator keeps for every family
// (both routes of prcg_update_values keep val current) gathers the diagonal blocks, inverts them and stores the device layout
int prcg_build_block_jacobi(prcg_t* h, int bs, int64_t* first_bad_block) {
    if (!h) return PRCG_EINVAL;
    if (first_bad_block) *first_bad_block = -1;
    CHECK(h, h->have_csr, "prcg_build_block_jacobi: no operator: call prcg_set_csr first");
    CHECK(h, bs >= 1 && bs <= 8, "prcg_build_block_jacobi: block size %d outside 1..8", bs);
    CHECK(h, h->g == 0, "prcg_build_block_jacobi: the operator is a row block with %lld ghost columns; the blocks are built for whole "
                        "operators on one GPU only (invert them on the host: prcg_set_block_jacobi)", (long long)h->g);
    CHECK(h, !h->multi() && h->nranks == 1, "prcg_build_block_jacobi: the handle has a communicator or a world size > 1; the blocks are "
                                            "built for whole operators on one GPU only");
    HIPCHK(h, hipSetDevice(h->dev));
    // the handle's pending work may still apply the old blocks
    HIPCHK(h, hipStreamSynchronize(h->sh));
    HIPCHK(h, hipStreamSynchronize(h->sm));
    HIPCHK(h, hipStreamSynchronize(h->sc));
    if (int rc = drop_block_jacobi(h)) return rc;
    const int64_t count = block_jacobi_layout(h->n, bs, nullptr, nullptr);
    HIPCHK(h, h->bj_blocks.alloc((size_t)count * sizeof(double), false));     // the kernel writes every entry
    if (!h->bj_flag.p) HIPCHK(h, h->bj_flag.alloc(sizeof(long long)));
    long long bad = INT64_MAX;
    HIPCHK(h, hipMemcpyAsync(h->bj_flag.p, &bad, sizeof bad, hipMemcpyHostToDevice, h->sc));
    HIPCHK(h, hipStreamSynchronize(h->sc));                                   // (`bad` is a pageable stack variable)
    if (launch_block_jacobi_build(h->sc, h->bj_blocks.d(), h->n, bs, h->indptr.i(), h->col.i(), h->val.d(),
                                  static_cast<long long*>(h->bj_flag.p)) != 0) {
        h->bj_blocks.release();
        return fail(h, PRCG_EHIP, "kernel launch failed (%s:%d)", __FILE__, __LINE__);
    }
    hipError_t e = hipMemcpyAsync(&bad, h->bj_flag.p, sizeof bad, hipMemcpyDeviceToHost, h->sc);
    if (e == hipSuccess) e = hipStreamSynchronize(h->sc);
    if (e != hipSuccess) {
        h->bj_blocks.release();
        return fail(h, PRCG_EHIP, "%s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
    }
    if (bad != INT64_MAX) {
        h->bj_blocks.release();                    // the handle is left without blocks
        if (first_bad_block) *first_bad_block = (int64_t)bad;
        return fail(h, PRCG_EINVAL, "prcg_build_block_jacobi: diagonal block %lld (bs = %d) is singular or not finite", bad, bs);
    }
    h->bj_bs = bs;
    h->cb = nullptr; h->cb_ctx = nullptr;          // the last preconditioner set is the one in force
    return PRCG_OK;
}

int prcg_get_block_jacobi(prcg_t* h, double* inv_blocks) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, !h->bj_var, "prcg_get_block_jacobi: the blocks on the handle have variable sizes: call prcg_get_block_jacobi_var");
    CHECK(h, h->bj_bs > 0, "prcg_get_block_jacobi: no block-Jacobi blocks on the handle (prcg_set_block_jacobi / prcg_build_block_jacobi)");
    CHECK(h, inv_blocks, "prcg_get_block_jacobi: null output");
    HIPCHK(h, hipSetDevice(h->dev));
    const int64_t count = block_jacobi_layout(h->n, h->bj_bs, nullptr, nullptr);
    std::vector<double> laid;
    try { laid.resize((size_t)count); } catch (const std::bad_alloc&) { return fail(h, PRCG_ENOMEM, "out of host memory"); }
    HIPCHK(h, hipStreamSynchronize(h->sc));
    if (count > 0) HIPCHK(h, hipMemcpy(laid.data(), h->bj_blocks.p, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
    block_jacobi_unlay(h->n, h->bj_bs, laid.data(), inv_blocks);
    return PRCG_OK;
}

// ---- blocks of variable size: the partition is checked and cut into tiles on the host (prcg_bjvar.h) BEFORE the handle is
// touched, so that a refusal leaves the blocks set before in force
static int bjvar_accept(prcg_t* h, const char* who, int64_t nb, const int64_t* block_ptr, BjVarPlan& P) {
    CHECK(h, block_ptr, "%s: null block_ptr", who);
    CHECK(h, nb >= 0, "%s: nb = %lld is negative", who, (long long)nb);
    int64_t k = 0, m = 0;
    switch (bjvar_check(h->n, nb, block_ptr, &k, &m)) {
    case 1: return fail(h, PRCG_EINVAL, "%s: block_ptr[0] is %lld, not 0", who, (long long)block_ptr[0]);
    case 2: return fail(h, PRCG_EINVAL, "%s: block_ptr[nb] is %lld, not n_rows = %lld", who, (long long)block_ptr[nb], (long long)h->n);
    case 3: return fail(h, PRCG_EINVAL, "%s: block %lld has size %lld, outside 1..8", who, (long long)k, (long long)m);
    default: break;
    }
    try {
        bjvar_plan(h->n, nb, block_ptr, P);
    } catch (const std::bad_alloc&) { return fail(h, PRCG_ENOMEM, "out of host memory"); }
    return PRCG_OK;
}

// the tables of an accepted partition onto the device, room for its blocks (not written here); the handle has no blocks before
static int bjvar_install(prcg_t* h, BjVarPlan& P, int64_t nb, const int64_t* block_ptr) {
    try { h->bjv_ptr.assign(block_ptr, block_ptr + nb + 1); } catch (const std::bad_alloc&) { return fail(h, PRCG_ENOMEM, "out of host memory"); }
    const size_t lanes = (size_t)P.ntiles * kBjvLanes;
    hipError_t e = h->bj_blocks.alloc((size_t)P.doubles() * sizeof(double), false);
    if (e == hipSuccess) e = h->bjv_tiles.alloc(P.tiles.size() * sizeof(int64_t), false);
    if (e == hipSuccess) e = h->bjv_bytes.alloc(2 * lanes, false);
    if (e == hipSuccess && lanes) e = hipMemcpy(h->bjv_tiles.p, P.tiles.data(), P.tiles.size() * sizeof(int64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && lanes) e = hipMemcpy(h->bjv_bytes.p, P.code.data(), lanes, hipMemcpyHostToDevice);
    if (e == hipSuccess && lanes) e = hipMemcpy(static_cast<unsigned char*>(h->bjv_bytes.p) + lanes, P.bidx.data(), lanes, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        h->bj_blocks.release(); h->bjv_tiles.release(); h->bjv_bytes.release(); h->bjv_ptr.clear();
        return fail(h, PRCG_EHIP, "%s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
    }
    h->bjv_plan = std::move(P);
    return PRCG_OK;
}

// the handle without blocks again after a failure behind bjvar_install
static void bjvar_abandon(prcg_t* h) {
    h->bj_blocks.release(); h->bjv_tiles.release(); h->bjv_bytes.release();
    h->bjv_plan = BjVarPlan{}; h->bjv_ptr.clear();
}

int prcg_set_block_jacobi_var(prcg_t* h, int64_t nb, const int64_t* block_ptr, const double* inv_blocks) {
    if (!h) return PRCG_EINVAL;
    if (!inv_blocks) return drop_block_jacobi(h);
    CHECK(h, h->have_csr, "prcg_set_block_jacobi_var: no operator: call prcg_set_csr first (the partition is checked against its n_rows)");
    CHECK(h, !h->multi(), "a block-Jacobi preconditioner runs on one GPU only");
    BjVarPlan P;
    if (int rc = bjvar_accept(h, "prcg_set_block_jacobi_var", nb, block_ptr, P)) return rc;
    std::vector<double> laid;
    try { laid.resize((size_t)P.doubles()); } catch (const std::bad_alloc&) { return fail(h, PRCG_ENOMEM, "out of host memory"); }
    bjvar_lay(P, block_ptr, inv_blocks, laid.data());
    if (int rc = drop_block_jacobi(h)) return rc;
    HIPCHK(h, hipSetDevice(h->dev));
    if (int rc = bjvar_install(h, P, nb, block_ptr)) return rc;
    if (!laid.empty()) {
        const hipError_t e = hipMemcpy(h->bj_blocks.p, laid.data(), laid.size() * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            bjvar_abandon(h);
            return fail(h, PRCG_EHIP, "%s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
        }
    }
    h->bj_var = true;
    h->cb = nullptr; h->cb_ctx = nullptr;        // the last preconditioner set is the one in force
    return PRCG_OK;
}

// prcg_build_block_jacobi for a partition: the same one pass over the caller-order CSR arrays, lane per row
int prcg_build_block_jacobi_var(prcg_t* h, int64_t nb, const int64_t* block_ptr, int64_t* first_bad_block) {
    if (!h) return PRCG_EINVAL;
    if (first_bad_block) *first_bad_block = -1;
    CHECK(h, h->have_csr, "prcg_build_block_jacobi_var: no operator: call prcg_set_csr first");
    BjVarPlan P;
    if (int rc = bjvar_accept(h, "prcg_build_block_jacobi_var", nb, block_ptr, P)) return rc;
    CHECK(h, h->g == 0, "prcg_build_block_jacobi_var: the operator is a row block with %lld ghost columns; the blocks are built for whole "
                        "operators on one GPU only (invert them on the host: prcg_set_block_jacobi_var)", (long long)h->g);
    CHECK(h, !h->multi() && h->nranks == 1, "prcg_build_block_jacobi_var: the handle has a communicator or a world size > 1; the blocks are "
                                            "built for whole operators on one GPU only");
    HIPCHK(h, hipSetDevice(h->dev));
    // the handle's pending work may still apply the old blocks
    HIPCHK(h, hipStreamSynchronize(h->sh));
    HIPCHK(h, hipStreamSynchronize(h->sm));
    HIPCHK(h, hipStreamSynchronize(h->sc));
    if (int rc = drop_block_jacobi(h)) return rc;
    if (!h->bj_flag.p) HIPCHK(h, h->bj_flag.alloc(sizeof(long long)));
    if (int rc = bjvar_install(h, P, nb, block_ptr)) return rc;         // the kernel writes every entry of the blocks
    long long bad = INT64_MAX;
    hipError_t e = hipMemcpyAsync(h->bj_flag.p, &bad, sizeof bad, hipMemcpyHostToDevice, h->sc);
    if (e == hipSuccess) e = hipStreamSynchronize(h->sc);                 // (`bad` is a pageable stack variable)
    if (e != hipSuccess) {
        bjvar_abandon(h);
        return fail(h, PRCG_EHIP, "%s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
    }
    if (launch_block_jacobi_var_build(h->sc, h->bj_blocks.d(), h->bjv_plan.ntiles, h->bjv_tiles_d(), h->bjv_code_d(), h->bjv_bidx_d(),
                                      h->indptr.i(), h->col.i(), h->val.d(), static_cast<long long*>(h->bj_flag.p)) != 0) {
        bjvar_abandon(h);
        return fail(h, PRCG_EHIP, "kernel launch failed (%s:%d)", __FILE__, __LINE__);
    }
    e = hipMemcpyAsync(&bad, h->bj_flag.p, sizeof bad, hipMemcpyDeviceToHost, h->sc);
    if (e == hipSuccess) e = hipStreamSynchronize(h->sc);
    if (e != hipSuccess) {
        bjvar_abandon(h);
        return fail(h, PRCG_EHIP, "%s (%s:%d)", hipGetErrorString(e), __FILE__, __LINE__);
    }
    if (bad != INT64_MAX) {
        bjvar_abandon(h);                          // the handle is left without blocks
        if (first_bad_block) *first_bad_block = (int64_t)bad;
        return fail(h, PRCG_EINVAL, "prcg_build_block_jacobi_var: diagonal block %lld (size %lld) is singular or not finite", bad,
                    (long long)(block_ptr[bad + 1] - block_ptr[bad]));
    }
    h->bj_var = true;
    h->cb = nullptr; h->cb_ctx = nullptr;          // the last preconditioner set is the one in force
    return PRCG_OK;
}

int prcg_get_block_jacobi_var(prcg_t* h, double* inv_blocks) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->bj_bs == 0, "prcg_get_block_jacobi_var: the blocks on the handle have one uniform size: call prcg_get_block_jacobi");
    CHECK(h, h->bj_var, "prcg_get_block_jacobi_var: no block-Jacobi blocks on the handle (prcg_set_block_jacobi_var / prcg_build_block_jacobi_var)");
    CHECK(h, inv_blocks, "prcg_get_block_jacobi_var: null output");
    HIPCHK(h, hipSetDevice(h->dev));
    const int64_t count = h->bjv_plan.doubles();
    std::vector<double> laid;
    try { laid.resize((size_t)count); } catch (const std::bad_alloc&) { return fail(h, PRCG_ENOMEM, "out of host memory"); }
    HIPCHK(h, hipStreamSynchronize(h->sc));
    if (count > 0) HIPCHK(h, hipMemcpy(laid.data(), h->bj_blocks.p, (size_t)count * sizeof(double), hipMemcpyDeviceToHost));
    bjvar_unlay(h->bjv_plan, h->bjv_ptr.data(), laid.data(), inv_blocks);
    return PRCG_OK;
}

int prcg_set_replace_hook(prcg_t* h, prcg_replace_fn fn, void* ctx) {
    if (!h) return PRCG_EINVAL;
    h->replace_fn = fn;
    h->replace_ctx = ctx;
    return PRCG_OK;
}

int prcg_set_option(prcg_t* h, const char* key, const char* value) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, key && value, "prcg_set_option: null key or value");
    CHECK(h, !h->have_csr, "prcg_set_option: options are fixed once the operator is set (call it before prcg_set_csr)");
    CHECK(h, apply_option(h->opt, key, value), "prcg_set_option: unknown option '%s'", key);
    return PRCG_OK;
}

int prcg_comm_unique_id(const char* rccl_path, void* id128) {
    if (!id128) return fail(nullptr, PRCG_EINVAL, "prcg_comm_unique_id: null buffer");
    std::string err;
    Rccl* r = Rccl::get(rccl_path, err);
    if (!r) return fail(nullptr, PRCG_ERCCL, "%s", err.c_str());
    ncclUniqueId id;
    ncclResult_t rc = r->GetUniqueId(&id);
    if (rc != ncclSuccess) return fail(nullptr, PRCG_ERCCL, "ncclGetUniqueId: %s", r->GetErrorString(rc));
    static_assert(sizeof(id) == 128, "ncclUniqueId is 128 bytes");
    memcpy(id128, &id, sizeof id);
    return PRCG_OK;
}

int prcg_comm_init(prcg_t* h, const char* rccl_path, int rank, int nranks, const void* id128, int n_ids) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, nranks >= 1 && rank >= 0 && rank < nranks, "prcg_comm_init: bad rank %d of %d", rank, nranks);
    CHECK(h, id128 != nullptr, "prcg_comm_init: null unique id");
    CHECK(h, n_ids == 1 || n_ids == 2, "prcg_comm_init: n_ids must be 1 or 2");
    CHECK(h, h->comm == nullptr, "prcg_comm_init: communicator already initialised");
    std::string err;
    h->rccl = Rccl::get(rccl_path, err);
    if (!h->rccl) return fail(h, PRCG_ERCCL, "%s", err.c_str());
    HIPCHK(h, hipSetDevice(h->dev));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof id);
    NCCLCHK(h, h->rccl->CommInitRank(&h->comm, nranks, id, rank));
    if (n_ids == 2) {
        memcpy(&id, static_cast<const char*>(id128) + sizeof id, sizeof id);
        NCCLCHK(h, h->rccl->CommInitRank(&h->comm_halo, nranks, id, rank));
    }
    h->rank = rank;
    h->nranks = nranks;
    return PRCG_OK;
}

// check arguments -> plan_operator (host only, prcg_plan.cpp) -> upload the plan's arrays -> keep its flags
int prcg_set_csr(prcg_t* h, int64_t n_rows, int64_t n_ghost, int64_t nnz, const void* indptr, int indptr_is64,
                 const int32_t* indices, const double* data) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, n_rows >= 0 && n_ghost >= 0 && nnz >= 0, "prcg_set_csr: negative size");
    CHECK(h, nnz < (int64_t)2147483000, "prcg_set_csr: nnz=%lld does not fit int32 row pointers", (long long)nnz);
    CHECK(h, n_rows + n_ghost < (int64_t)2147483000, "prcg_set_csr: too many rows for int32 column indices");
    CHECK(h, indptr && (nnz == 0 || (indices && data)), "prcg_set_csr: null array");
    h->in_session = false;   // a new operator invalidates any open session
    HIPCHK(h, hipSetDevice(h->dev));
    if (int rc = drop_block_jacobi(h)) return rc;     // ... and drops block-Jacobi blocks, sized for the old one

    // --- validate on the host before anything reaches a kernel, then decide family and encodings ---
    std::vector<int32_t> ip;
    if (int rc = checked_indptr(h, n_rows, nnz, indptr, indptr_is64, ip)) return rc;
    if (int rc = install_operator(h, n_rows, n_ghost, nnz, ip.data(), indices, data)) return rc;
    h->have_halo = false;
    h->gather_planned = false;
    return PRCG_OK;
}

// New values on the pattern prcg_set_csr fixed: in place where no encoding holds values (values_route, prcg_plan.cpp), else the
// operator is planned and uploaded again from the pattern read back and the new values
int prcg_update_values(prcg_t* h, const double* data, int data_on_device) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->have_csr, "prcg_update_values: no operator: call prcg_set_csr first");
    CHECK(h, data_on_device == 0 || data_on_device == 1, "prcg_update_values: data_on_device = %d is neither 0 (host) nor 1 (device)", data_on_device);
    CHECK(h, h->g == 0, "prcg_update_values: the operator is a row block with %lld ghost columns; only whole operators on one GPU are updated "
                        "(set the block again with prcg_set_csr)", (long long)h->g);
    CHECK(h, !h->multi() && h->nranks == 1, "prcg_update_values: the handle has a communicator or a world size > 1; only whole operators on one GPU "
                                            "are updated (set the block again with prcg_set_csr)");
    CHECK(h, data || h->nnz == 0, "prcg_update_values: null data");
    if (h->nnz == 0) return PRCG_OK;
    const int64_t n = h->n, nnz = h->nnz;
    const size_t bytes = (size_t)nnz * sizeof(double);
    HIPCHK(h, hipSetDevice(h->dev));
    if (data_on_device) {
        CHECK(h, reinterpret_cast<uintptr_t>(data) % sizeof(double) == 0, "prcg_update_values: device pointer %p is not aligned to 8 bytes", (const void*)data);
        if (int rc = checked_device_range(h, "prcg_update_values", data, bytes)) return rc;
    }
    // the handle's pending work reads the old values
    HIPCHK(h, hipStreamSynchronize(h->sh));
    HIPCHK(h, hipStreamSynchronize(h->sm));
    HIPCHK(h, hipStreamSynchronize(h->sc));
    if (values_route(*h) == 0) {
        // the plan stays: values in the caller's order (window tiles with plain values and CSR-adaptive tiles read them), and
        // for sliced rows the re-laid copy rewritten from them
        HIPCHK(h, hipMemcpyAsync(h->val.p, data, bytes, data_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->sc));
        HIPCHK(h, hipStreamSynchronize(h->sc));             // `data` has been read: the caller may overwrite it
        h->in_session = false;                              // new values invalidate any open session
        if (h->sell) {
            const int grid = launch_sell_set_values(h->sc, h->sdev(), h->sslice_ptr(0), h->nst_int + h->nst_bnd, h->val.d(),
                                                    static_cast<double*>(h->sval.p));
            if (grid < 0) return fail(h, PRCG_EHIP, "kernel launch failed (%s:%d)", __FILE__, __LINE__);
        }
        return PRCG_OK;
    }
    // a dictionary or pattern tiles hold values: prcg_set_csr's plan and upload under the handle's options, with the pattern
    // read back from the device (no host copy is kept) -- preconditioners and session buffers stay
    std::vector<int32_t> ip, idx;
    std::vector<double> host;
    try {
        ip.resize((size_t)n + 1); idx.resize((size_t)nnz);
        if (data_on_device) host.resize((size_t)nnz);
    } catch (const std::bad_alloc&) { return fail(h, PRCG_ENOMEM, "out of host memory"); }
    HIPCHK(h, hipMemcpy(ip.data(), h->indptr.p, ((size_t)n + 1) * sizeof(int32_t), hipMemcpyDeviceToHost));
    HIPCHK(h, hipMemcpy(idx.data(), h->col.p, (size_t)nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (data_on_device) HIPCHK(h, hipMemcpy(host.data(), data, bytes, hipMemcpyDeviceToHost));
    h->in_session = false;
    return install_operator(h, n, 0, nnz, ip.data(), idx.data(), data_on_device ? host.data() : data);
}

int prcg_values_route(const prcg_t* h) { return (h && h->have_csr) ? values_route(*h) : -1; }

int prcg_set_halo(prcg_t* h, int n_peers, const int32_t* peer_rank, const int64_t* send_ptr, const int32_t* send_idx,
                  const int64_t* recv_ptr) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->have_csr, "prcg_set_halo: call prcg_set_csr first");
    CHECK(h, n_peers >= 0 && (n_peers == 0 || (peer_rank && send_ptr && recv_ptr)), "prcg_set_halo: null array");
    HIPCHK(h, hipSetDevice(h->dev));
    h->n_peers = n_peers;
    h->peer_rank.assign(peer_rank, peer_rank + n_peers);
    h->send_ptr.assign(1, 0);
    h->recv_ptr.assign(1, 0);
    if (n_peers > 0) {
        h->send_ptr.assign(send_ptr, send_ptr + n_peers + 1);
        h->recv_ptr.assign(recv_ptr, recv_ptr + n_peers + 1);
    }
    CHECK(h, h->send_ptr[0] == 0 && h->recv_ptr[0] == 0, "prcg_set_halo: pointers must start at 0");
    for (int q = 0; q < n_peers; ++q) {
        // peer == own rank is allowed: RCCL does self send/recv inside a group, which is how
        // the one-GPU tests drive the whole halo path (loopback ghosts)
        CHECK(h, h->peer_rank[q] >= 0 && h->peer_rank[q] < h->nranks, "prcg_set_halo: bad peer rank %d",
              h->peer_rank[q]);
        CHECK(h, h->send_ptr[q + 1] >= h->send_ptr[q] && h->recv_ptr[q + 1] >= h->recv_ptr[q],
              "prcg_set_halo: pointers not monotone");
    }
    CHECK(h, h->recv_ptr[n_peers] == h->g, "prcg_set_halo: receive counts (%lld) != n_ghost (%lld)",
          (long long)h->recv_ptr[n_peers], (long long)h->g);
    const int64_t nsend = h->send_ptr[n_peers];
    for (int64_t j = 0; j < nsend; ++j)
        CHECK(h, send_idx[j] >= 0 && send_idx[j] < h->n, "prcg_set_halo: send index %d out of range", send_idx[j]);
    HIPCHK(h, h->send_idx.alloc((size_t)(nsend + 1) * sizeof(int32_t)));
    HIPCHK(h, h->send_buf.alloc((size_t)(nsend + 1) * 2 * sizeof(double)));
    if (nsend > 0)
        HIPCHK(h, hipMemcpy(h->send_idx.p, send_idx, (size_t)nsend * sizeof(int32_t), hipMemcpyHostToDevice));
    h->send_idx_host.assign(send_idx, send_idx + nsend);
    h->peer_ok = false;
    h->have_halo = true;
    h->gather_planned = false;
    return PRCG_OK;
}

int prcg_peer_setup(prcg_t* h, int64_t max_ghost_any_rank, void* ipc_handle64, void** local_ptr) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->have_csr, "prcg_peer_setup: call prcg_set_csr (and prcg_set_halo) first");
    CHECK(h, h->nranks >= 1 && h->nranks <= kMaxPeerRanks, "prcg_peer_setup: 1..%d ranks", kMaxPeerRanks);
    CHECK(h, max_ghost_any_rank >= h->g && max_ghost_any_rank < (int64_t)1 << 28, "prcg_peer_setup: ghost capacity %lld < this rank's %lld ghosts",
          (long long)max_ghost_any_rank, (long long)h->g);
    HIPCHK(h, hipSetDevice(h->dev));
    h->peer_ok = false;
    const size_t bytes = peer_buffer_doubles(h->nranks, (int)max_ghost_any_rank) * sizeof(double) + 4096;
    if (!h->xbuf || h->xbuf_bytes < bytes || h->ghost_cap != (int)max_ghost_any_rank) {
        CHECK(h, h->peer_opened.empty() && !h->xbuf, "prcg_peer_setup: the exchange buffer of a connected handle cannot change size");
        // fine-grained device memory: stores of OTHER GPUs become visible to this one's loads without a kernel boundary
        h->xbuf_fine = hipExtMallocWithFlags(&h->xbuf, bytes, hipDeviceMallocFinegrained) == hipSuccess;
        if (!h->xbuf_fine) {
            (void)hipGetLastError();
            HIPCHK(h, hipMalloc(&h->xbuf, bytes));
        }
        h->xbuf_bytes = bytes;
        h->ghost_cap = (int)max_ghost_any_rank;
        HIPCHK(h, hipMemset(h->xbuf, 0, bytes));
        HIPCHK(h, hipDeviceSynchronize());
    }
    if (ipc_handle64) {
        static_assert(sizeof(hipIpcMemHandle_t) == 64, "the C-ABI hands IPC handles around as 64 bytes");
        hipIpcMemHandle_t hd;
        memset(&hd, 0, sizeof hd);
        if (hipIpcGetMemHandle(&hd, h->xbuf) != hipSuccess) { (void)hipGetLastError(); memset(&hd, 0, sizeof hd); }   // same-process peers still work
        memcpy(ipc_handle64, &hd, sizeof hd);
    }
    if (local_ptr) *local_ptr = h->xbuf;
    return PRCG_OK;
}

int prcg_peer_connect(prcg_t* h, const void* ipc_handles, void* const* same_process_ptrs, const int64_t* send_dst_off) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->xbuf != nullptr, "prcg_peer_connect: call prcg_peer_setup first");
    CHECK(h, h->g == 0 || h->have_halo, "prcg_peer_connect: ghost columns but no halo plan");
    const int np = h->have_halo ? h->n_peers : 0;
    CHECK(h, np == 0 || send_dst_off != nullptr, "prcg_peer_connect: null destination offsets");
    HIPCHK(h, hipSetDevice(h->dev));
    h->peer_ok = false;
    const int R = h->nranks;
    PeerDev& P = h->peer_host;
    if (h->peer_opened.empty()) {
        for (int q = 0; q < kMaxPeerRanks; ++q) P.peer[q] = nullptr;
        for (int q = 0; q < R; ++q) {
            if (q == h->rank) { P.peer[q] = static_cast<double*>(h->xbuf); continue; }
            if (same_process_ptrs && same_process_ptrs[q]) { P.peer[q] = static_cast<double*>(same_process_ptrs[q]); continue; }
            CHECK(h, ipc_handles != nullptr, "prcg_peer_connect: no handle for rank %d", q);
            hipIpcMemHandle_t hd;
            memcpy(&hd, static_cast<const char*>(ipc_handles) + (size_t)q * sizeof hd, sizeof hd);
            void* mapped = nullptr;
            hipError_t e = hipIpcOpenMemHandle(&mapped, hd, hipIpcMemLazyEnablePeerAccess);
            if (e != hipSuccess)
                return fail(h, PRCG_EHIP, "hipIpcOpenMemHandle for rank %d's exchange buffer: %s", q, hipGetErrorString(e));
            h->peer_opened.push_back(mapped);
            P.peer[q] = static_cast<double*>(mapped);
        }
    }
    P.mine = static_cast<double*>(h->xbuf);
    P.rank = h->rank; P.nranks = R; P.n_own = (int)h->n; P.ghost_cap = h->ghost_cap; P.epoch = 0;
    // send entries {row, destination rank, index in its ghost area}, grouped by the tile that owns the row
    struct Ent { int32_t row, peer, dst, tile; };
    std::vector<Ent> ents;
    if (h->win && np > 0) {
        const size_t nt = h->wt_rb.size();
        std::vector<int32_t> order(nt);
        for (size_t i = 0; i < nt; ++i) order[i] = (int32_t)i;
        std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return h->wt_rb[a] < h->wt_rb[b]; });
        for (int q = 0; q < np; ++q) {
            const int64_t cnt = h->send_ptr[q + 1] - h->send_ptr[q];
            CHECK(h, send_dst_off[q] >= 0 && send_dst_off[q] + cnt <= h->ghost_cap,
                  "prcg_peer_connect: rows for rank %d would land outside its ghost area", h->peer_rank[q]);
            for (int64_t j = 0; j < cnt; ++j) {
                const int32_t row = h->send_idx_host[(size_t)(h->send_ptr[q] + j)];
                // the tile whose rows hold `row`: last tile (by first row) that starts at or before it
                size_t lo = 0, hi = nt;
                while (hi - lo > 1) { const size_t mid = (lo + hi) / 2; if (h->wt_rb[order[mid]] <= row) lo = mid; else hi = mid; }
                const int32_t t = order[lo];
                CHECK(h, row >= h->wt_rb[t] && row < h->wt_re[t], "prcg_peer_connect: row %d lies in no tile", row);
                ents.push_back(Ent{row, h->peer_rank[q], (int32_t)(send_dst_off[q] + j), t});
            }
        }
        std::stable_sort(ents.begin(), ents.end(), [](const Ent& a, const Ent& b) { return a.tile != b.tile ? a.tile < b.tile : a.row < b.row; });
    }
    const size_t nt = h->wt_rb.size();
    std::vector<int32_t> tsend(2 * (nt + 1), 0), flat(4 * (ents.size() + 1), 0);
    {
        size_t e = 0;
        for (size_t t = 0; t < nt; ++t) {
            tsend[2 * t] = (int32_t)e;
            while (e < ents.size() && ents[e].tile == (int32_t)t) ++e;
            tsend[2 * t + 1] = (int32_t)e;
        }
        for (size_t i = 0; i < ents.size(); ++i) { flat[4 * i] = ents[i].row; flat[4 * i + 1] = ents[i].peer; flat[4 * i + 2] = ents[i].dst; }
    }
    HIPCHK(h, h->peer_tile_send.alloc(tsend.size() * sizeof(int32_t)));
    HIPCHK(h, hipMemcpy(h->peer_tile_send.p, tsend.data(), tsend.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(h, h->peer_ents.alloc(flat.size() * sizeof(int32_t)));
    HIPCHK(h, hipMemcpy(h->peer_ents.p, flat.data(), flat.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(h, h->peer_dev.alloc(sizeof(PeerDev)));
    P.tile_send = static_cast<const int2*>(h->peer_tile_send.p);
    P.send_ent = static_cast<const int4*>(h->peer_ents.p);
    P.n_send = (int)ents.size();
    HIPCHK(h, hipMemcpy(h->peer_dev.p, &P, sizeof P, hipMemcpyHostToDevice));
    if (h->win) {
        launch_flag_send_tiles(h->sc, h->wtiles.p, h->peer_tile_send.p, (int)nt);
        HIPCHK(h, hipStreamSynchronize(h->sc));
    }
    // (a non-window operator keeps the two-kernel schedule: the exchange is the iteration launch's own, and only the
    //  window kernels have it)
    h->peer_ok = h->win;
    return PRCG_OK;
}

int prcg_world_init(prcg_t* h, int rank, int nranks) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, nranks >= 1 && rank >= 0 && rank < nranks, "prcg_world_init: bad rank %d of %d", rank, nranks);
    CHECK(h, h->comm == nullptr, "prcg_world_init: the handle already has a communicator");
    h->rank = rank;
    h->nranks = nranks;
    return PRCG_OK;
}

int prcg_peer_selftest(prcg_t* h, int k, const double* rows2n, const double* slot5, double* sums5, double* ghost2g) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->peer_ok, "prcg_peer_selftest: call prcg_peer_setup / prcg_peer_connect first");
    CHECK(h, k >= 0 && rows2n && slot5 && sums5, "prcg_peer_selftest: bad argument");
    HIPCHK(h, hipSetDevice(h->dev));
    const PeerDev* px = static_cast<const PeerDev*>(h->peer_dev.p);
    DevBuf rows, slot, out, err;
    HIPCHK(h, rows.alloc((size_t)2 * (h->n + 1) * sizeof(double)));
    HIPCHK(h, slot.alloc(64));
    HIPCHK(h, out.alloc(64));
    HIPCHK(h, err.alloc(64));
    HIPCHK(h, hipMemcpy(rows.p, rows2n, (size_t)2 * h->n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(slot.p, slot5, 5 * sizeof(double), hipMemcpyHostToDevice));
    if (h->peer_host.epoch == 0) {
        h->peer_host.epoch = (unsigned long long)(++h->peer_epoch) << 32;
        HIPCHK(h, hipMemcpy(h->peer_dev.p, &h->peer_host, sizeof(PeerDev), hipMemcpyHostToDevice));
    }
    launch_peer_push(h->sc, px, rows.d(), slot.d(), k, 1);
    launch_peer_collect(h->sc, px, k, nullptr, 0, out.d(), nullptr, static_cast<unsigned*>(err.p));
    HIPCHK(h, hipStreamSynchronize(h->sc));
    unsigned e = 0;
    HIPCHK(h, hipMemcpy(&e, err.p, sizeof e, hipMemcpyDeviceToHost));
    if (e) return fail(h, PRCG_ERCCL, "prcg_peer_selftest: the other ranks' slots of round %d did not arrive", k);
    HIPCHK(h, hipMemcpy(sums5, out.p, 5 * sizeof(double), hipMemcpyDeviceToHost));
    if (ghost2g && h->g > 0)
        HIPCHK(h, hipMemcpy(ghost2g, static_cast<const double*>(h->xbuf) + peer_ghost_off(h->nranks, h->ghost_cap, k & 1),
                            (size_t)2 * h->g * sizeof(double), hipMemcpyDeviceToHost));
    return PRCG_OK;
}

static int timed_product(prcg_t* h, int nc, const double* in, double* out, int reps, double* ms_avg) {
    CHECK(h, h->have_csr, "no matrix: call prcg_set_csr first");
    CHECK(h, in && out && reps >= 1, "bad argument");
    CHECK(h, h->g == 0 || (h->multi() && h->have_halo), "ghost columns need a communicator and a halo plan");
    HIPCHK(h, hipSetDevice(h->dev));
    int rc = h2d(h, h->tmp_ext.d(), in, h->n * nc);
    if (rc) return rc;
    if ((rc = exchange(h, h->tmp_ext.d(), nc, h->sc))) return rc;
    hipEvent_t a, b;
    HIPCHK(h, hipEventCreate(&a));
    HIPCHK(h, hipEventCreate(&b));
    double total = 0.0;
    for (int i = 0; i < reps; ++i) {
        HIPCHK(h, hipEventRecord(a, h->sc));
        if (nc == 1)
            LAUNCHCHK(h, eng_spmv(h, h->sc, 0, h->tmp_ext.d(), h->t1.d(), kEpiNone, nullptr, nullptr, nullptr, nullptr));
        else
            LAUNCHCHK(h, eng_spmm2(h, h->sc, 0, h->tmp_ext.d(), h->t1.d(), 3));
        HIPCHK(h, hipEventRecord(b, h->sc));
        HIPCHK(h, hipEventSynchronize(b));
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, a, b));
        total += ms;
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    if (ms_avg) *ms_avg = total / reps;
    return d2h(h, out, h->t1.d(), h->n * nc);
}

int prcg_spmv(prcg_t* h, const double* x, double* y, int reps, double* ms_avg) {
    if (!h) return PRCG_EINVAL;
    return timed_product(h, 1, x, y, reps, ms_avg);
}

int prcg_stream_ceiling(prcg_t* h, int64_t n_pairs, int mode, int reps, double* gbytes_per_s) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, n_pairs >= 1024 && mode >= 0 && mode <= 3 && reps >= 1 && gbytes_per_s, "prcg_stream_ceiling: bad argument");
    HIPCHK(h, hipSetDevice(h->dev));
    DevBuf a, b, c;
    const size_t bytes = (size_t)n_pairs * 16;
    HIPCHK(h, a.alloc(bytes));
    const bool mix = mode == 1 || mode == 2;
    HIPCHK(h, b.alloc(mix ? bytes : 64));
    HIPCHK(h, c.alloc(mix ? bytes : 64));
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0));
    HIPCHK(h, hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) launch_stream_probe(h->sc, mode, a.d(), b.d(), c.d(), (size_t)n_pairs);
    HIPCHK(h, hipEventRecord(e0, h->sc));
    for (int i = 0; i < reps; ++i) launch_stream_probe(h->sc, mode, a.d(), b.d(), c.d(), (size_t)n_pairs);
    HIPCHK(h, hipEventRecord(e1, h->sc));
    HIPCHK(h, hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    const double moved = (double)bytes * (mix ? 4.0 : 1.0) * reps;
    *gbytes_per_s = ms > 0.f ? moved / (ms * 1e-3) * 1e-9 : 0.0;
    return PRCG_OK;
}

int prcg_mix_ceiling(prcg_t* h, int64_t n_rows, int stream_kb_per_64_rows, int reps, double* gbytes_per_s) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, n_rows >= 4096 && stream_kb_per_64_rows >= 0 && stream_kb_per_64_rows <= 256 && reps >= 1 && gbytes_per_s, "prcg_mix_ceiling: bad argument");
    HIPCHK(h, hipSetDevice(h->dev));
    DevBuf v, x, r, rn;
    const size_t pieces = (size_t)n_rows / 64;
    const size_t vbytes = (pieces + 1) * (size_t)stream_kb_per_64_rows * 1024 + 4096, pbytes = ((size_t)n_rows + 64) * 16;
    HIPCHK(h, v.alloc(vbytes));
    HIPCHK(h, x.alloc(pbytes));
    HIPCHK(h, r.alloc(pbytes));
    HIPCHK(h, rn.alloc(pbytes));
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0));
    HIPCHK(h, hipEventCreate(&e1));
    for (int i = 0; i < 2; ++i) launch_stream_mix(h->sc, v.d(), x.d(), r.d(), rn.d(), (size_t)n_rows, stream_kb_per_64_rows);
    HIPCHK(h, hipEventRecord(e0, h->sc));
    for (int i = 0; i < reps; ++i) launch_stream_mix(h->sc, v.d(), x.d(), r.d(), rn.d(), (size_t)n_rows, stream_kb_per_64_rows);
    HIPCHK(h, hipEventRecord(e1, h->sc));
    HIPCHK(h, hipEventSynchronize(e1));
    float ms = 0.f;
    HIPCHK(h, hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    const double moved = ((double)pieces * stream_kb_per_64_rows * 1024.0 + 64.0 * (double)pieces * 64.0) * reps;
    *gbytes_per_s = ms > 0.f ? moved / (ms * 1e-3) * 1e-9 : 0.0;
    return PRCG_OK;
}

int prcg_spmv_ext(prcg_t* h, const double* x_ext, double* y) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->have_csr, "no matrix: call prcg_set_csr first");
    CHECK(h, x_ext && y, "bad argument");
    HIPCHK(h, hipSetDevice(h->dev));
    int rc = h2d(h, h->tmp_ext.d(), x_ext, h->n + h->g);
    if (rc) return rc;
    // interior tiles, then the tiles that touch ghost columns: the two launches of the overlapped schedule
    LAUNCHCHK(h, eng_spmv(h, h->sc, 1, h->tmp_ext.d(), h->t1.d(), kEpiNone, nullptr, nullptr, nullptr, nullptr));
    LAUNCHCHK(h, eng_spmv(h, h->sc, 2, h->tmp_ext.d(), h->t1.d(), kEpiNone, nullptr, nullptr, nullptr, nullptr));
    return d2h(h, y, h->t1.d(), h->n);
}

int prcg_spmm2(prcg_t* h, const double* rs, double* wu, int reps, double* ms_avg) {
    if (!h) return PRCG_EINVAL;
    return timed_product(h, 2, rs, wu, reps, ms_avg);
}

int prcg_spmm4(prcg_t* h, const double* x4, double* y4, int reps, double* ms_avg) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->have_csr, "no matrix: call prcg_set_csr first");
    CHECK(h, x4 && y4 && reps >= 1, "bad argument");
    CHECK(h, !h->multi() && h->g == 0, "prcg_spmm4: one GPU, whole operators only (no communicator, n_ghost = 0)");
    HIPCHK(h, hipSetDevice(h->dev));
    const int64_t n = h->n;
    const size_t D = sizeof(double);
    HIPCHK(h, h->x4b.ensure((size_t)2 * (n + kGatherPad) * D, h->sc));
    HIPCHK(h, h->y4b.ensure((size_t)2 * n * D, h->sc));
    std::vector<double> pairs;
    try { pairs.resize((size_t)2 * n); } catch (const std::bad_alloc&) { return fail(h, PRCG_ENOMEM, "prcg_spmm4: host staging"); }
    int rc;
    for (int g = 0; g < 2; ++g) {
        for (int64_t i = 0; i < n; ++i) { pairs[2 * i] = x4[4 * i + 2 * g]; pairs[2 * i + 1] = x4[4 * i + 2 * g + 1]; }
        if ((rc = h2d(h, g == 0 ? h->tmp_ext.d() : h->x4b.d(), pairs.data(), 2 * n))) return rc;
    }
    hipEvent_t a, b;
    HIPCHK(h, hipEventCreate(&a));
    HIPCHK(h, hipEventCreate(&b));
    double total = 0.0;
    for (int i = 0; i < reps; ++i) {
        HIPCHK(h, hipEventRecord(a, h->sc));
        LAUNCHCHK(h, eng_spmm4(h, h->sc, 0, h->tmp_ext.d(), h->x4b.d(), h->t1.d(), h->y4b.d()));
        HIPCHK(h, hipEventRecord(b, h->sc));
        HIPCHK(h, hipEventSynchronize(b));
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, a, b));
        total += ms;
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    if (ms_avg) *ms_avg = total / reps;
    for (int g = 0; g < 2; ++g) {
        if ((rc = d2h(h, pairs.data(), g == 0 ? h->t1.d() : h->y4b.d(), 2 * n))) return rc;
        for (int64_t i = 0; i < n; ++i) { y4[4 * i + 2 * g] = pairs[2 * i]; y4[4 * i + 2 * g + 1] = pairs[2 * i + 1]; }
    }
    return PRCG_OK;
}

// What the row results of a one-launch iteration cost beside the operator's read stream depends on WHERE the written arrays lie:
// the same byte mix runs at two speeds from process to process (tools/mixbench.hip: s4b's mix 467-477 or 530-560 us, the read
// stream alone 443 either way; r04_sweeps.md D, K) and from allocation to allocation inside a process.  The session's three
// large arrays -- (x,p), the (r,s) pairs and their second copy -- are therefore allocated k times, every placement is timed with
// the mix probe against the operator's own stream (k_stream_mix: reads of the stream, reads of two pair arrays, nontemporal
// writes of two), and the fastest is kept.  A few milliseconds per placement, once per handle (the allocations are kept for
// later sessions).  Buffers are zeroed again afterwards; nothing has been written into them yet.
int place_session_vectors(prcg_t* h, size_t xp_bytes, size_t rs_bytes) {
    const int64_t n = h->n;
    const double* stream = nullptr;
    size_t stream_bytes = 0;
    if (h->sell) { stream = h->val_sell(); stream_bytes = h->sval.bytes; }
    else if (h->val.p && h->val.bytes >= (size_t)h->nnz * 8) { stream = h->val.d(); stream_bytes = (size_t)h->nnz * 8; }
    const size_t pieces = (size_t)n / 64;
    if (pieces < 4096 || rs_bytes < (size_t)n * 16 || xp_bytes < (size_t)n * 16) return PRCG_OK;      // (262,144 rows and more: smaller sessions are launch-bound)
    // KB of stream per 64 rows, so that the probe stays inside the stream's allocation (and a dictionary operator: none)
    int kb = 0;
    if (stream && !(h->win && (h->win_vd || h->win_pat))) {
        kb = (int)std::min<size_t>(stream_bytes / (pieces + 1) / 1024, 200);
    }
    if (kb == 0) stream = h->xp.d();               // (the probe's first loads read one line of it)
    hipEvent_t e0, e1;
    HIPCHK(h, hipEventCreate(&e0));
    HIPCHK(h, hipEventCreate(&e1));
    auto probe = [&](double* xp, double* rs, double* rs2, float* ms) -> int {
        launch_stream_mix(h->sc, stream, xp, rs, rs2, (size_t)n, kb);
        HIPCHK(h, hipEventRecord(e0, h->sc));
        for (int i = 0; i < 3; ++i) launch_stream_mix(h->sc, stream, xp, rs, rs2, (size_t)n, kb);
        HIPCHK(h, hipEventRecord(e1, h->sc));
        HIPCHK(h, hipEventSynchronize(e1));
        HIPCHK(h, hipEventElapsedTime(ms, e0, e1));
        return PRCG_OK;
    };
    float best = 0.f;
    int rc = probe(h->xp.d(), h->rs.d(), h->rs2.d(), &best);
    if (rc) return rc;
    if (getenv("PRCG_PLAN_DEBUG")) fprintf(stderr, "place_session_vectors: placement 0: %.1f us (stream %d KB per 64 rows)\n", best / 3 * 1e3, kb);
    // (every placement stays allocated until the choice is made: a freed one would be handed out again for the next)
    std::vector<std::array<DevBuf, 3>> cand((size_t)h->opt.place_k - 1);
    int best_c = -1;
    for (int c = 0; c + 1 < h->opt.place_k; ++c) {
        DevBuf& cx = cand[(size_t)c][0]; DevBuf& cr = cand[(size_t)c][1]; DevBuf& cr2 = cand[(size_t)c][2];
        if (cx.alloc(xp_bytes, false) != hipSuccess || cr.alloc(rs_bytes, false) != hipSuccess || cr2.alloc(rs_bytes, false) != hipSuccess) {
            (void)hipGetLastError();                 // (no room for another placement: the ones so far compete; the error is not the session's)
            break;
        }
        HIPCHK(h, hipMemsetAsync(cx.p, 0, xp_bytes, h->sc));
        HIPCHK(h, hipMemsetAsync(cr.p, 0, rs_bytes, h->sc));
        HIPCHK(h, hipMemsetAsync(cr2.p, 0, rs_bytes, h->sc));
        float ms = 0.f;
        if ((rc = probe(cx.d(), cr.d(), cr2.d(), &ms))) return rc;
        if (getenv("PRCG_PLAN_DEBUG")) fprintf(stderr, "place_session_vectors: placement %d: %.1f us\n", c + 1, ms / 3 * 1e3);
        if (ms < best) { best = ms; best_c = c; }
    }
    if (best_c >= 0) {
        DevBuf& cx = cand[(size_t)best_c][0]; DevBuf& cr = cand[(size_t)best_c][1]; DevBuf& cr2 = cand[(size_t)best_c][2];
        std::swap(h->xp.p, cx.p); std::swap(h->xp.cap, cx.cap); std::swap(h->xp.bytes, cx.bytes);
        std::swap(h->rs.p, cr.p); std::swap(h->rs.cap, cr.cap); std::swap(h->rs.bytes, cr.bytes);
        std::swap(h->rs2.p, cr2.p); std::swap(h->rs2.cap, cr2.cap); std::swap(h->rs2.bytes, cr2.bytes);
    }
    cand.clear();                                   // (the others are freed)
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    HIPCHK(h, hipMemsetAsync(h->xp.p, 0, h->xp.bytes, h->sc));
    HIPCHK(h, hipMemsetAsync(h->rs.p, 0, h->rs.bytes, h->sc));
    HIPCHK(h, hipMemsetAsync(h->rs2.p, 0, h->rs2.bytes, h->sc));
    h->placed_xp = h->xp.p;
    return PRCG_OK;
}

}  // extern "C"

namespace {

// ---- session start --------------------------------------------------------------------------------------------
// Every session is opened here, whichever family it belongs to: the shared argument checks, THE reset of the session state
// (the only assignment of Session{}), the fields every family fills the same way, the caller's leading vectors (`lead`:
// allocated before the scalar arrays, as they always were -- the order of hipMalloc decides where a vector lies), then
// dinv, dots and coef, and the profiling sample counts.  The session stays closed (in_session false) until its family
// has computed the initial state.
struct Lead { DevBuf* buf; size_t bytes; };
int open_session(prcg_t* h, const char* who, int variant, int max_iter, uint32_t hist_mask, const double* inv_diag, bool have_xtrue,
                 std::initializer_list<Lead> lead, int rows_per_iteration = 1) {
    CHECK(h, h->have_csr, "%s: call prcg_set_csr first", who);
    CHECK(h, max_iter >= 1, "%s: max_iter must be >= 1", who);
    HIPCHK(h, hipSetDevice(h->dev));
    static_cast<Session&>(*h) = Session{};
    Session& s = *h;
    s.variant = variant;
    s.bj_session = h->have_block_jacobi() && inv_diag == nullptr;
    s.stored_tilde = (h->cb != nullptr || s.bj_session) && inv_diag == nullptr;
    s.prec = inv_diag != nullptr || s.stored_tilde;
    CHECK(h, !(s.stored_tilde && h->multi()), "a host-callback or block-Jacobi preconditioner runs on one GPU only");
    if (s.stored_tilde && !s.bj_session) HIPCHK(h, h->cb_stage.ensure((size_t)h->n * sizeof(double), h->sc));
    s.max_iter = max_iter;
    s.hist_mask = hist_mask;
    s.have_xtrue = have_xtrue;
    h->n_ev_spmv = h->n_ev_upd = 0;
    const size_t D = sizeof(double);
    for (const Lead& l : lead) HIPCHK(h, l.buf->ensure(l.bytes, h->sc));
    // every vector that feeds a matrix product has ghost room AND kGatherPad spare entries (dinv is a window source of
    // the Chronopoulos-Gear product launch)
    HIPCHK(h, h->dinv.ensure((size_t)(h->n + h->g + kGatherPad) * D, h->sc));
    // (rows_per_iteration = 2: the predict-and-recompute two-RHS session keeps one scalar and one coefficient row per column;
    //  four right-hand sides: twice the rows again, one set per pair group)
    HIPCHK(h, h->dots.ensure((size_t)(max_iter + 1) * rows_per_iteration * kNS * D, h->sc));
    HIPCHK(h, h->coef.ensure((size_t)(max_iter + 1) * rows_per_iteration * kCoefStride * D, h->sc));
    if (inv_diag) return h2d(h, h->dinv.d(), inv_diag, h->n);
    return PRCG_OK;
}

}  // namespace

extern "C" {

int prcg_solve_begin(prcg_t* h, int variant, const double* b, const double* x0, int max_iter, const double* x_true,
                     const double* inv_diag, uint32_t hist_mask) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, variant >= 0 && variant < PRCG_NUM_VARIANTS, "prcg_solve_begin: unknown variant %d", variant);
    CHECK(h, b && x0, "prcg_solve_begin: null b or x0");
    CHECK(h, (hist_mask & ~PRCG_HIST_ALL) == 0, "prcg_solve_begin: unknown history bits");
    CHECK(h, !(hist_mask & (PRCG_HIST_ERROR_A_NORM | PRCG_HIST_ERROR_2_NORM)) || x_true,
          "prcg_solve_begin: error histories need x_true");
    CHECK(h, h->g == 0 || (h->multi() && h->have_halo), "ghost columns need a communicator and a halo plan");
    // every vector that feeds a matrix product has ghost room AND kGatherPad spare entries: the
    // narrow column encodings decode a few out-of-tile bytes per tile against the tile's own base
    // (products nobody reads); the pad keeps those gathers inside the allocation without a test
    const int64_t n = h->n, ne = h->n + h->g + kGatherPad;
    const size_t D = sizeof(double);
    int rc = open_session(h, "prcg_solve_begin", variant, max_iter, hist_mask, inv_diag, x_true != nullptr,
                          {{&h->x, (size_t)n * D}, {&h->b, (size_t)n * D}, {&h->xt, (size_t)n * D}, {&h->e_ext, (size_t)ne * D}});
    if (rc) return rc;
    if ((rc = h2d(h, h->x.d(), x0, n))) return rc;
    if ((rc = h2d(h, h->b.d(), b, n))) return rc;
    if (x_true && (rc = h2d(h, h->xt.d(), x_true, n))) return rc;
    hipStream_t sc = h->sc;
    double* tmp = h->tmp_ext.d();
    double* t1 = h->t1.d();

    // r0 = b - A x0   (hs_cg.py:23, pipe_pr_cg.py:23)
    launch_copy(sc, tmp, 1, h->x.d(), 1, n);
    if ((rc = dist_spmv(h, tmp, t1, kEpiNone, nullptr, nullptr, nullptr, nullptr))) return rc;

    if (is_pipe(variant)) {
        h->fused = h->opt.want_fused && !h->multi() && h->g == 0 && !h->stored_tilde;
        // direct peer exchange (every rank connected, window operator): the one-launch schedule without a collective.
        // Whether it is connected is the same on every rank (the host side connects all ranks or none).
        h->peer = h->peer_ok && h->opt.want_peer && h->opt.want_fused && h->multi() && h->win && !h->stored_tilde;
        if (!h->peer && (rc = plan_gather(h))) return rc;
        // with a communicator: the same kernel in its deferred form -- window operators whose halo rides on the
        // one all-gather per iteration (bands; the merged exchange).  Larger halos (send/recv + all-reduce chain)
        // keep the two-kernel schedule: RCCL's point-to-point path was seen to stall for ~1 s on its first use
        // from the communication stream while a launch waited for it (profiles/r02_sweeps.md).
        // (the one-launch schedule over the RCCL all-gather chain is opt-in, PRCG_FUSED_COMM=1: its launches wait inside the
        //  kernel for kernels of ANOTHER stream to become resident, which has only ever been validated with one rank)
        h->fused_comm = h->peer || (h->opt.want_fused && h->opt.want_fused_comm_rccl && h->multi() && h->win && h->gather);
        if (h->fused_comm) h->fused = true;        // state layout, derived vectors: as the one-launch schedule
        HIPCHK(h, h->xp.ensure((size_t)2 * n * D, h->sc));
        HIPCHK(h, h->rs.ensure((size_t)2 * (h->prec ? n : ne) * D, h->sc));
        HIPCHK(h, h->rs2.ensure((h->fused && !h->prec) ? (size_t)2 * ne * D : 16, h->sc));
        if (h->opt.place_k > 1 && h->fused && !h->prec && h->placed_xp != h->xp.p && h->rs.bytes == h->rs2.bytes) {       // (every rank for itself: its vectors are its own)
            int prc = place_session_vectors(h, h->xp.bytes, h->rs.bytes);
            if (prc) return prc;
        }
        HIPCHK(h, h->rst2.ensure((h->fused && h->prec) ? (size_t)2 * ne * D : 16, h->sc));
        HIPCHK(h, h->wv.ensure((h->fused && !pipe_recompute(variant)) ? (size_t)n * D : 16, h->sc));
        HIPCHK(h, h->partC.ensure(h->fused ? (size_t)8192 * kPartialStride * sizeof(double) : 16, h->sc));
        HIPCHK(h, h->pub.ensure(h->fused_comm ? kPubDoubles * sizeof(double) : 16, h->sc));
        HIPCHK(h, h->pub_err.ensure(64, h->sc));
        h->rs_cur = h->rs.d();
        // one-workgroup solver: only when nothing but the recurrence residual is recorded
        h->small = h->fused && !h->fused_comm && h->opt.want_small && !h->prec && pipe_recompute(variant) &&
                   !records_state(hist_mask) &&
                   small_fits(h->n, h->nnz, h->max_row_len, &h->small_mode);
        HIPCHK(h, h->rst.ensure(h->prec ? (size_t)2 * ne * D : 16, h->sc));
        if (h->prec) h->rs_cur = h->rst.d();
        HIPCHK(h, h->wu.ensure((size_t)2 * n * D, h->sc));
        HIPCHK(h, h->wt.ensure(h->prec ? (size_t)n * D : 16, h->sc));
        HIPCHK(h, h->ut.ensure(h->stored_tilde ? (size_t)n * D : 16, h->sc));
        double* RS = h->rs.d();
        double* WU = h->wu.d();
        double* XP = h->xp.d();
        launch_copy(sc, XP, 2, h->x.d(), 1, n);                             // x = x0         :22
        launch_sub(sc, RS, 2, h->b.d(), 1, t1, 1, n);                       // r = b - A x
        if (!h->prec) {
            launch_copy(sc, XP + 1, 2, RS, 2, n);                           // p = r          :24
            launch_copy(sc, tmp, 1, RS, 2, n);
            if ((rc = dist_spmv(h, tmp, t1, kEpiNone, nullptr, nullptr, nullptr, nullptr))) return rc;
            launch_copy(sc, RS + 1, 2, t1, 1, n);                           // s = A p        :26
            launch_copy(sc, WU, 2, t1, 1, n);                               // w = s          :27
            launch_copy(sc, tmp, 1, t1, 1, n);
            if ((rc = dist_spmv(h, tmp, t1, kEpiNone, nullptr, nullptr, nullptr, nullptr))) return rc;
            launch_copy(sc, WU + 1, 2, t1, 1, n);                           // u = A w        :28
        } else {
            double* RST = h->rst.d();
            if ((rc = apply_prec(h, RS, 2, RST, 2))) return rc;            // r~ = M^-1 r    :124
            launch_copy(sc, XP + 1, 2, RST, 2, n);                          // p = r~         :125
            launch_copy(sc, tmp, 1, RST, 2, n);
            if ((rc = dist_spmv(h, tmp, t1, kEpiNone, nullptr, nullptr, nullptr, nullptr))) return rc;
            launch_copy(sc, RS + 1, 2, t1, 1, n);                           // s = A p        :127
            if ((rc = apply_prec(h, t1, 1, RST + 1, 2))) return rc;        // s~ = M^-1 s    :128
            launch_copy(sc, WU, 2, t1, 1, n);                               // w = s          :129
            launch_copy(sc, h->wt.d(), 1, RST + 1, 2, n);                   // w~ = s~        :130
            launch_copy(sc, tmp, 1, RST + 1, 2, n);
            if ((rc = dist_spmv(h, tmp, t1, kEpiNone, nullptr, nullptr, nullptr, nullptr))) return rc;
            launch_copy(sc, WU + 1, 2, t1, 1, n);                           // u = A s~       :131
            if (h->stored_tilde && (rc = apply_prec(h, WU + 1, 2, h->ut.d(), 1))) return rc;   // u~ = M^-1 u  :132
        }
        if (h->fused && !pipe_recompute(variant)) launch_copy(sc, h->wv.d(), 1, WU, 2, n);   // the stored w of the 'p' flavours
        PipeUpdateArgs a = pipe_args(h, 0);
        const int grid = launch_pipe_dots(sc, a);                           // nu, mu, delta, gamma
        LAUNCHCHK(h, grid);
        launch_reduce_final(sc, h->partA.d(), grid, dots_at(h, 0), 0, 0, 5);
        if ((rc = allreduce(h, dots_at(h, 0), 5, sc))) return rc;
        if (h->gather) {
            // COLLECTIVE part, the same on every rank of a merged-exchange session whatever schedule the rank itself
            // ends up with (a rank's block may be no window operator, or its probe below may fail: the ranks then
            // still issue the same collectives in the same order -- one all-gather per iteration either way):
            // the first use of the communicator from the communication stream happens HERE, not inside a launch that
            // waits for it, and the ghosts of the initial input pairs are in place for the first boundary tiles.
            HIPCHK(h, hipStreamSynchronize(sc));
            double* slot = h->gbuf.d() + (size_t)h->rank * h->g_slot;
            NCCLCHK(h, h->rccl->AllGather(slot, h->gbuf.p, (size_t)h->g_slot, ncclDouble, h->comm, h->sm));
            HIPCHK(h, hipStreamSynchronize(h->sm));
            if ((rc = exchange(h, h->rs_cur, 2, sc))) return rc;
        }
        if (h->peer) {
            // The initial state into the exchange buffers: this rank's boundary rows into the neighbours' ghost areas and its
            // slot of "iteration 0" (rank 0 carries the reduced inner products).  Ordered behind the all-reduce above on this
            // stream, i.e. behind everything the neighbours still had in flight from an earlier session on theirs.
            h->peer_host.epoch = (unsigned long long)(++h->peer_epoch) << 32;
            h->peer_host.n_own = (int)h->n;
            HIPCHK(h, hipMemcpyAsync(h->peer_dev.p, &h->peer_host, sizeof(PeerDev), hipMemcpyHostToDevice, sc));
            HIPCHK(h, hipStreamSynchronize(sc));                       // (peer_host must not change under the copy)
            *h->err_host = 0u;
            launch_peer_push(sc, static_cast<const PeerDev*>(h->peer_dev.p), h->rs_cur, dots_at(h, 0), 0, h->rank == 0);
            launch_peer_collect(sc, static_cast<const PeerDev*>(h->peer_dev.p), 0, nullptr, 0, nullptr, h->pub.d(), static_cast<unsigned*>(h->pub_err.p));
        } else if (h->fused_comm) {
            // LOCAL part.  Can a kernel of the communication stream run while a kernel of the compute stream waits for
            // it?  (HIP may have mapped both streams to one hardware queue -- then the deferred form would only ever
            // time out.)  Probe once per session: a one-wave kernel on sc waits ~2 ms at most for a record that a
            // kernel on sm publishes.
            HIPCHK(h, hipStreamSynchronize(sc));
            launch_probe_wait(sc, h->pub.d(), 0x7f000000u, static_cast<unsigned*>(h->pub_err.p));
            launch_publish(h->sm, dots_at(h, 0), h->pub.d(), 0x7f000000u);
            HIPCHK(h, hipStreamSynchronize(h->sm));
            HIPCHK(h, hipStreamSynchronize(sc));
            unsigned perr = 0;
            HIPCHK(h, hipMemcpy(&perr, h->pub_err.p, sizeof perr, hipMemcpyDeviceToHost));
            HIPCHK(h, hipMemset(h->pub_err.p, 0, sizeof perr));
            if (perr) { h->fused_comm = false; h->fused = false; }       // streams are serialised here: two-kernel schedule
        }
        if (h->fused_comm && !h->peer) launch_publish(sc, dots_at(h, 0), h->pub.d(), 0u);   // iteration 1 waits for "0": the initial inner products
    } else if (is_cg_family(variant)) {
        // x, r, r~, w, w~ (all with ghost room: whichever feeds the SpMV), p, s, s~, u, t
        HIPCHK(h, h->p.ensure((size_t)ne * D, h->sc));
        h->p_cur = h->p.d();
        HIPCHK(h, h->r.ensure((size_t)ne * D, h->sc));
        h->cur_r = h->r.d();
        h->cg_fused = h->opt.want_fused && !h->multi() && h->g == 0 && h->win && !h->stored_tilde &&
                      !(variant == PRCG_GV && h->replace_fn);      // (the predicate is called between the update and the product)
        // one launch per iteration: both variants unpreconditioned, Chronopoulos-Gear with Jacobi too
        h->cg_one = h->cg_fused && h->opt.want_cg_one && (variant == PRCG_CG_CG || !h->prec);
        HIPCHK(h, h->r2.ensure((h->cg_fused && variant == PRCG_CG_CG) ? (size_t)ne * D : 16, h->sc));
        HIPCHK(h, h->w2.ensure((h->cg_fused && (variant == PRCG_GV || h->cg_one)) ? (size_t)ne * D : 16, h->sc));
        HIPCHK(h, h->s2.ensure((h->cg_one && variant == PRCG_CG_CG) ? (size_t)ne * D : 16, h->sc));
        HIPCHK(h, h->u2.ensure((h->cg_one && variant == PRCG_GV) ? (size_t)ne * D : 16, h->sc));
        HIPCHK(h, h->t2.ensure((h->cg_one && variant == PRCG_GV) ? (size_t)ne * D : 16, h->sc));
        HIPCHK(h, h->partC.ensure(h->cg_one ? (size_t)8192 * kPartialStride * sizeof(double) : 16, h->sc));
        HIPCHK(h, h->rt.ensure(h->prec ? (size_t)ne * D : 16, h->sc));
        HIPCHK(h, h->w.ensure((size_t)ne * D, h->sc));
        h->cur_w = h->w.d();
        HIPCHK(h, h->wt.ensure(h->prec ? (size_t)ne * D : 16, h->sc));
        HIPCHK(h, h->s.ensure((size_t)ne * D, h->sc));
        HIPCHK(h, h->st.ensure(h->prec ? (size_t)n * D : 16, h->sc));
        HIPCHK(h, h->u.ensure((size_t)ne * D, h->sc));      // (a window source of the Ghysels-Vanroose product launch)
        HIPCHK(h, h->tvec.ensure((size_t)ne * D, h->sc));   // (... of its one-launch form)
        h->cur_s = h->s.d(); h->cur_u = h->u.d(); h->cur_t = h->tvec.d();
        launch_sub(sc, h->r.d(), 1, h->b.d(), 1, t1, 1, n);                 // r = b - A x      cg_cg.py:23
        if (h->prec && (rc = apply_prec(h, h->r.d(), 1, h->rt.d(), 1))) return rc;   // r~ = M^-1 r   :89
        double* z = h->prec ? h->rt.d() : h->r.d();
        launch_copy(sc, h->p.d(), 1, z, 1, n);                              // p = r~           :25 / :91
        int grid = 0;
        if (variant == PRCG_CG_CG) {
            // w = A r~ with nu = r.r~, eta = w.r~ (:24,26,27); s = A p with mu = p.s (:28,30)
            if ((rc = dist_spmv(h, z, h->w.d(), kEpiCG, h->r.d(), nullptr, nullptr, &grid))) return rc;
            launch_reduce_final(sc, h->partB.d(), grid, dots_at(h, 0), 0, 0, 5);
            if ((rc = dist_spmv(h, h->p.d(), h->s.d(), kEpiDotXY, nullptr, nullptr, nullptr, &grid))) return rc;
            launch_reduce_final(sc, h->partB.d(), grid, dots_at(h, 0), 0, PRCG_S_MU, 1);
            if ((rc = allreduce(h, dots_at(h, 0), 5, sc))) return rc;
        } else {
            // gv_cg.py:26-33 / gv_pcg :96-109
            if ((rc = dist_spmv(h, z, h->w.d(), kEpiNone, nullptr, nullptr, nullptr, nullptr))) return rc;   // w = A r~
            if (h->prec && (rc = apply_prec(h, h->w.d(), 1, h->wt.d(), 1))) return rc;                         // w~
            launch_copy(sc, h->s.d(), 1, h->w.d(), 1, n);                                                      // s = w
            if (h->prec) launch_copy(sc, h->st.d(), 1, h->wt.d(), 1, n);                                       // s~ = w~
            double* zt = h->prec ? h->wt.d() : h->w.d();
            if ((rc = dist_spmv(h, zt, h->u.d(), kEpiNone, nullptr, nullptr, nullptr, nullptr))) return rc;  // u = A w~
            CgArgs a = cg_args(h, 0);
            const int g1 = launch_gv_update1(sc, a, true);                                                     // nu, eta
            LAUNCHCHK(h, g1);
            launch_reduce_final(sc, h->partA.d(), g1, dots_at(h, 0), 0, 0, 5);
            // mu = p.s as a true inner product at the start (gv_cg.py:33)
            const int g2 = launch_dot(sc, h->p.d(), h->s.d(), n, h->partB.d(), 0);
            LAUNCHCHK(h, g2);
            launch_reduce_final(sc, h->partB.d(), g2, dots_at(h, 0), 0, PRCG_S_MU, 1);
            if ((rc = allreduce(h, dots_at(h, 0), 5, sc))) return rc;
        }
    } else {
        // HS and non-pipelined PR share the layout x, r, (r~), p(+ghosts), s, (s~)
        HIPCHK(h, h->p.ensure((size_t)ne * D, h->sc));
        h->p_cur = h->p.d();
        h->hs_fused = variant == PRCG_HS && h->opt.want_fused && !h->multi() && h->g == 0 && !h->stored_tilde;
        // one-workgroup solver (k_small_hs): only when nothing but the recurrence residual is recorded
        h->small_hs = h->hs_fused && h->opt.want_small && !h->prec &&
                      !records_state(hist_mask) &&
                      small_fits(h->n, h->nnz, h->max_row_len, &h->small_mode);
        // r (r~) is the staged-window source of the Hestenes-Stiefel product launch: like every vector that feeds a
        // product it has the spare entries behind its end (a window page of the last tile may reach past row n)
        HIPCHK(h, h->r.ensure((size_t)(h->opt.debug_short_sources ? n : ne) * D, h->sc));
        HIPCHK(h, h->s.ensure((size_t)ne * D, h->sc));
        HIPCHK(h, h->rt.ensure(h->prec ? (size_t)ne * D : 16, h->sc));
        HIPCHK(h, h->st.ensure(h->prec ? (size_t)ne * D : 16, h->sc));
        // one launch per iteration for pr / m on a window operator: second copies of what the window is formed from
        h->pr_fused = is_pr(variant) && h->opt.want_fused && !h->multi() && h->g == 0 && h->win && !h->stored_tilde;
        HIPCHK(h, h->p2.ensure(((h->hs_fused && h->win) || h->pr_fused) ? (size_t)ne * D : 16, h->sc));
        HIPCHK(h, h->r2.ensure((h->pr_fused && !h->prec) ? (size_t)ne * D : 16, h->sc));
        HIPCHK(h, h->s2.ensure((h->pr_fused && !h->prec) ? (size_t)ne * D : 16, h->sc));
        HIPCHK(h, h->rt2.ensure((h->pr_fused && h->prec) ? (size_t)ne * D : 16, h->sc));
        HIPCHK(h, h->st2.ensure((h->pr_fused && h->prec) ? (size_t)ne * D : 16, h->sc));
        HIPCHK(h, h->partC.ensure(h->pr_fused ? (size_t)8192 * kPartialStride * sizeof(double) : 16, h->sc));
        h->pr_packed = h->pr_fused && (h->opt.want_pr_pack < 0 ? h->win_pat : h->opt.want_pr_pack != 0) && !h->prec &&
                       !records_state(hist_mask);
        HIPCHK(h, h->q.ensure(h->pr_packed ? (size_t)4 * ne * D : 16, h->sc));
        HIPCHK(h, h->q2.ensure(h->pr_packed ? (size_t)4 * ne * D : 16, h->sc));
        h->cur_r = h->r.d(); h->cur_s = h->s.d(); h->cur_rt = h->rt.d(); h->cur_st = h->st.d();
        launch_sub(sc, h->r.d(), 1, h->b.d(), 1, t1, 1, n);                 // r = b - A x
        if (h->prec) {
            if ((rc = apply_prec(h, h->r.d(), 1, h->rt.d(), 1))) return rc;   // r~ = M^-1 r
            launch_copy(sc, h->p.d(), 1, h->rt.d(), 1, n);                  // p = r~
        } else {
            launch_copy(sc, h->p.d(), 1, h->r.d(), 1, n);                   // p = r
        }
        if (variant == PRCG_HS) {
            HsArgs a = hs_args(h, 0);
            const int g1 = launch_hs_init_dots(sc, a);                      // nu = r.r~      hs_cg.py:25
            LAUNCHCHK(h, g1);
            launch_reduce_final(sc, h->partA.d(), g1, dots_at(h, 0), PRCG_S_NU, PRCG_S_NU, 2);
            if (h->stored_tilde) {        // nu = r~.r with the r~ the callback returned
                const int g2 = launch_dot(sc, h->rt.d(), h->r.d(), n, h->partB.d(), 0);
                LAUNCHCHK(h, g2);
                launch_reduce_final(sc, h->partB.d(), g2, dots_at(h, 0), 0, PRCG_S_NU, 1);
            }
            if ((rc = allreduce(h, dots_at(h, 0) + PRCG_S_NU, 2, sc))) return rc;
            int grid = 0;
            if ((rc = dist_spmv(h, h->p.d(), h->s.d(), kEpiDotXY, nullptr, nullptr, nullptr, &grid))) return rc;
            launch_reduce_final(sc, h->partB.d(), grid, dots_at(h, 0), 0, PRCG_S_MU, 1);   // mu = p.s  :27
            if ((rc = allreduce(h, dots_at(h, 0) + PRCG_S_MU, 1, sc))) return rc;
        } else {
            PrArgs a = pr_args(h, 0);
            const int g1 = launch_pr_init_dots(sc, a);                      // nu = r~.r      pr_cg.py:109
            LAUNCHCHK(h, g1);
            int grid = 0;
            if (h->stored_tilde) {
                if ((rc = pr_spmv_and_reduce(h, 0, g1))) return rc;                       // (s~ from the callback)
            } else {
                if ((rc = dist_spmv(h, h->p.d(), h->s.d(), kEpiPR, h->r.d(), h->prec ? h->dinv.d() : nullptr,
                                    h->prec ? h->st.d() : nullptr, &grid))) return rc;    // s, s~, mu, dl, gm
                launch_reduce_final(sc, h->partA.d(), g1, dots_at(h, 0), PRCG_S_NU, PRCG_S_NU, 2);
                launch_reduce_final(sc, h->partB.d(), grid, dots_at(h, 0), 0, 0, 3);
                if ((rc = allreduce(h, dots_at(h, 0), 5, sc))) return rc;
            }
        }
    }
    if ((rc = record(h, 0))) return rc;
    HIPCHK(h, hipStreamSynchronize(sc));
    h->in_session = true;
    return PRCG_OK;
}

int prcg_iterate(prcg_t* h, int iters) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->in_session, "prcg_iterate: no open session");
    CHECK(h, iters >= 0, "prcg_iterate: negative count");
    CHECK(h, h->k + iters <= h->max_iter, "prcg_iterate: %d more iterations exceed max_iter=%d (k=%d)", iters,
          h->max_iter, h->k);
    HIPCHK(h, hipSetDevice(h->dev));
    if (h->fused_comm && *h->err_host != 0u)
        return fail(h, PRCG_ERCCL, "a one-launch iteration waited more than its bound for the other ranks (a peer stalled or died); "
                                   "the session's results are invalid -- PRCG_PEER=0 / PRCG_FUSED_COMM=0 select the two-kernel schedule");
    if (h->rhs2) {
        for (int i = 0; i < iters; ++i) {
            const int rc = h->pipe2 ? iterate_pipe2(h, h->k + 1) : pr2(h) ? iterate_pr2(h, h->k + 1) : iterate_hs2(h, h->k + 1);
            if (rc) return rc;
            ++h->k;
        }
        return PRCG_OK;
    }
    if (h->small_hs && iters > 0) {
        // Hestenes-Stiefel: all `iters` iterations inside one launch of one workgroup
        hs_flush(h);
        SmallArgs sa{};
        sa.n = (int)h->n; sa.nnz = (int)h->nnz;
        sa.indptr = h->indptr.i(); sa.col = h->col.i(); sa.val = h->val.d();
        sa.xp = h->x.d(); sa.rs = h->r.d(); sa.hs_p = h->p_cur; sa.hs_s = h->s.d();
        sa.dots = h->dots.d(); sa.coef = h->coef.d();
        sa.k0 = h->k; sa.iters = iters; sa.meurant = 0;
        bool on = false;
        prof_begin(h, h->ev_spmv, h->n_ev_spmv, 0, on);
        LAUNCHCHK(h, launch_small_hs(h->sc, sa, h->small_mode));
        prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
        h->k += iters;
        return PRCG_OK;
    }
    if (h->small && iters > 0) {
        // all `iters` iterations inside one launch of one workgroup
        SmallArgs sa{};
        sa.n = (int)h->n; sa.nnz = (int)h->nnz;
        sa.indptr = h->indptr.i(); sa.col = h->col.i(); sa.val = h->val.d();
        sa.xp = h->xp.d(); sa.rs = h->rs_cur;
        sa.dots = h->dots.d(); sa.coef = h->coef.d();
        sa.k0 = h->k; sa.iters = iters; sa.meurant = meurant(h->variant);
        bool on = false;
        prof_begin(h, h->ev_spmv, h->n_ev_spmv, 0, on);
        LAUNCHCHK(h, launch_small_pipe_pr(h->sc, sa, h->small_mode));
        prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
        h->k += iters;
        return PRCG_OK;
    }
    // deferred (x,p) store: (SKIP, APPLY) pairs counted from the start of the call, an odd last launch closes itself --
    // when the loop ends the arrays in memory are current
    const int n_paired = xp_deferred(h) ? (iters & ~1) : 0;
    for (int i = 0; i < iters; ++i) {
        const int k = h->k + 1;
        int rc;
        h->xphase = i < n_paired ? 1 + (i & 1) : 0;
        if (is_pipe(h->variant)) rc = iterate_pipe(h, k);
        else if (h->variant == PRCG_HS) rc = h->hs_fused ? iterate_hs_fused(h, k) : iterate_hs(h, k);
        else if (is_cg_family(h->variant) && h->cg_one) rc = iterate_cg_one(h, k);
        else if (h->variant == PRCG_CG_CG) rc = h->cg_fused ? iterate_cgcg_fused(h, k) : iterate_cgcg(h, k);
        else if (h->variant == PRCG_GV) rc = h->cg_fused ? iterate_gv_fused(h, k) : iterate_gv(h, k);
        else rc = h->pr_fused ? iterate_pr_fused(h, k) : iterate_pr(h, k);
        if (rc) return rc;
        if ((rc = record(h, k))) return rc;
        h->k = k;
    }
    h->xphase = 0;
    // dots of the last iteration: one reduction per call, not per iteration; the caller may read or rewrite state next
    if (int rc = flush_pending(h)) return rc;
    return PRCG_OK;
}

int prcg_sync(prcg_t* h) {
    if (!h) return PRCG_EINVAL;
    HIPCHK(h, hipSetDevice(h->dev));
    HIPCHK(h, hipStreamSynchronize(h->sh));
    HIPCHK(h, hipStreamSynchronize(h->sm));
    HIPCHK(h, hipStreamSynchronize(h->sc));
    if (h->in_session && h->fused_comm && h->pub_err.p) {
        unsigned err = 0;
        HIPCHK(h, hipMemcpy(&err, h->pub_err.p, sizeof err, hipMemcpyDeviceToHost));
        if (err) *h->err_host = 1u;
        if (err) return fail(h, PRCG_ERCCL, "a one-launch iteration waited more than its bound for the reduced inner products "
                                            "(communication stream starved or a peer stalled); results are invalid. "
                                            "PRCG_FUSED_COMM=0 selects the two-kernel schedule");
    }
    return PRCG_OK;
}

int prcg_iteration(const prcg_t* h) { return h ? h->k : -1; }

int64_t prcg_operator_bytes(const prcg_t* h) { return (h && h->have_csr) ? h->bytes() : -1; }

int prcg_schedule(const prcg_t* h) {
    if (!h) return -1;
    return ((h->fused || h->hs_fused || h->pr_fused || h->cg_fused) ? PRCG_SCHED_FUSED : 0) | (h->fused_comm ? PRCG_SCHED_FUSED_COMM : 0) |
           (h->peer ? PRCG_SCHED_PEER : 0) | (h->sell ? PRCG_SCHED_SELL | PRCG_SCHED_COL16 : 0) | ((h->small || h->small_hs) ? PRCG_SCHED_SMALL : 0) | (h->comm ? PRCG_SCHED_COMM : 0) |
           (h->gather ? PRCG_SCHED_GATHER : 0) | (h->comm_halo ? PRCG_SCHED_DUAL_COMM : 0) | ((h->steps & 15) << 8) |
           (h->stream_stores ? PRCG_SCHED_STREAM_STORES : 0) | (h->bj_session ? PRCG_SCHED_BLOCK_JACOBI : 0) | ((h->bj_session && h->bj_var) ? PRCG_SCHED_BLOCK_JACOBI_VAR : 0) | ((h->sell && h->sell_sigma > 64) ? PRCG_SCHED_SELL_SORTED : 0) |
           (xp_deferred(h) ? PRCG_SCHED_XP_DEFERRED : 0) | ((h->rhs2 && h->groups == 1) ? PRCG_SCHED_RHS2 : 0) |
           (h->groups == 2 ? PRCG_SCHED_RHS4 : 0) | (h->spmm4 ? PRCG_SCHED_SPMM4 : 0) | (h->pipe2 ? PRCG_SCHED_RHS2_PIPE : 0) |
           ((h->sell && h->sell_nt) ? PRCG_SCHED_NT_LOADS : 0) | ((h->sell && h->sell_window > 0) ? PRCG_SCHED_SELL_WINDOW : 0) |
           ((h->win ? h->win_vd : h->vd_int) ? PRCG_SCHED_VALDICT : 0) |
           (h->win ? (h->win_pat ? PRCG_SCHED_PATTERN : (h->win_geom < 2 ? PRCG_SCHED_COL8 : PRCG_SCHED_COL16)) | PRCG_SCHED_WINDOW
                   : (h->c8_int ? PRCG_SCHED_COL8 : (h->c16_int ? PRCG_SCHED_COL16 : 0)));
}

int prcg_set_iteration(prcg_t* h, int k) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->in_session, "prcg_set_iteration: no open session");
    NOT_RHS2(h, "prcg_set_iteration");
    CHECK(h, k >= 0 && k < h->max_iter, "prcg_set_iteration: k out of range");
    h->k = k;
    if (h->peer && is_pipe(h->variant)) {
        // teacher forcing: the exchange buffers must describe the state just loaded -- rows and slot of "iteration k" again
        int rc = prcg_sync(h);
        if (rc) return rc;
        if ((rc = allreduce(h, h->t1.d(), 1, h->sc))) return rc;      // (collective: nobody is still reading what the pushes overwrite)
        launch_peer_push(h->sc, static_cast<const PeerDev*>(h->peer_dev.p), h->rs_cur, dots_at(h, k), k, h->rank == 0);
        launch_peer_collect(h->sc, static_cast<const PeerDev*>(h->peer_dev.p), k, nullptr, 0, nullptr, h->pub.d(), static_cast<unsigned*>(h->pub_err.p));
        HIPCHK(h, hipStreamSynchronize(h->sc));
        h->pend_parts = 0;
        return PRCG_OK;
    }
    if (h->gather && is_pipe(h->variant)) {
        // teacher forcing: what the deferred launch of iteration k+1 waits for and what its boundary tiles read
        // must describe the state just loaded (the exchange is collective over the session's ranks)
        int rc = prcg_sync(h);
        if (rc) return rc;
        if (h->fused_comm) launch_publish(h->sc, dots_at(h, k), h->pub.d(), (unsigned)k);
        if ((rc = exchange(h, h->fused ? h->rs_cur : (h->prec ? h->rst.d() : h->rs.d()), 2, h->sc))) return rc;
        HIPCHK(h, hipStreamSynchronize(h->sc));
        h->red_pending = false;
    }
    return PRCG_OK;
}

int prcg_get_vector(prcg_t* h, int which, double* out) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->in_session && out, "prcg_get_vector: no session or null buffer");
    NOT_RHS2(h, "prcg_get_vector");
    int rc = prcg_sync(h);
    if (rc) return rc;
    const int64_t n = h->n;
    double* base; int stride;
    if (!locate(h, which, &base, &stride)) {
        // fused schedule: u = A s (A s~) and, in the 'pr' flavours, w = A r (A r~) are never stored --
        // recompute on request from the current SpMM input pairs
        const bool tilde = is_pipe(h->variant) && h->prec && (which == PRCG_VEC_UT || which == PRCG_VEC_WT);
        if (h->fused && (which == PRCG_VEC_W || which == PRCG_VEC_U || tilde))
            LAUNCHCHK(h, eng_spmm2(h, h->sc, 0, h->rs_cur, h->wu.d(), 3));
        if (h->fused && (which == PRCG_VEC_W || which == PRCG_VEC_U)) {
            launch_copy(h->sc, h->t1.d(), 1, h->wu.d() + (which == PRCG_VEC_U ? 1 : 0), 2, n);
            return d2h(h, out, h->t1.d(), n);
        }
        // derived tilde vectors of the Jacobi 'pr' flavours: w~ = M^-1 w, u~ = M^-1 u
        if (tilde) {
            launch_mul(h->sc, h->t1.d(), 1, h->dinv.d(), 1, h->wu.d() + (which == PRCG_VEC_UT ? 1 : 0), 2, n);
            return d2h(h, out, h->t1.d(), n);
        }
        return fail(h, PRCG_EINVAL, "prcg_get_vector: vector %d is not part of variant %d", which, h->variant);
    }
    if (stride == 1) return d2h(h, out, base, n);
    launch_copy(h->sc, h->t1.d(), 1, base, stride, n);
    return d2h(h, out, h->t1.d(), n);
}

int prcg_set_vector(prcg_t* h, int which, const double* in) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->in_session && in, "prcg_set_vector: no session or null buffer");
    NOT_RHS2(h, "prcg_set_vector");
    int rc = prcg_sync(h);
    if (rc) return rc;
    const int64_t n = h->n;
    double* base; int stride;
    if (!locate(h, which, &base, &stride)) {
        if (h->fused && (which == PRCG_VEC_W || which == PRCG_VEC_U)) return PRCG_OK;                          // derived
        if (is_pipe(h->variant) && h->prec && (which == PRCG_VEC_UT || which == PRCG_VEC_WT)) return PRCG_OK;  // derived
        return fail(h, PRCG_EINVAL, "prcg_set_vector: vector %d is not part of variant %d", which, h->variant);
    }
    if (stride == 1) return h2d(h, base, in, n);
    if ((rc = h2d(h, h->t1.d(), in, n))) return rc;
    launch_copy(h->sc, base, stride, h->t1.d(), 1, n);
    HIPCHK(h, hipStreamSynchronize(h->sc));
    return PRCG_OK;
}

int prcg_get_scalars(prcg_t* h, int k, double* out) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->in_session && out && k >= 0 && k <= h->max_iter, "prcg_get_scalars: bad argument");
    NOT_RHS2(h, "prcg_get_scalars");
    int rc = prcg_sync(h);
    if (rc) return rc;
    return d2h(h, out, dots_at(h, k), kNS);
}

int prcg_set_scalars(prcg_t* h, int k, const double* in) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->in_session && in && k >= 0 && k <= h->max_iter, "prcg_set_scalars: bad argument");
    NOT_RHS2(h, "prcg_set_scalars");
    int rc = prcg_sync(h);
    if (rc) return rc;
    if ((rc = h2d(h, dots_at(h, k), in, kNS))) return rc;
    if (h->peer) return PRCG_OK;      // (prcg_set_iteration re-sends rows and slot once the whole state is loaded)
    if (h->fused_comm) {      // the deferred launch of iteration k+1 reads the published copy
        launch_publish(h->sc, dots_at(h, k), h->pub.d(), (unsigned)k);
        HIPCHK(h, hipStreamSynchronize(h->sc));
    }
    return PRCG_OK;
}

int prcg_get_coefficients(prcg_t* h, int k, double* out) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->in_session && out && k >= 1 && k <= h->max_iter, "prcg_get_coefficients: bad argument");
    NOT_RHS2(h, "prcg_get_coefficients");
    int rc = prcg_sync(h);
    if (rc) return rc;
    return d2h(h, out, coef_at(h, k), 3);
}

int prcg_get_history(prcg_t* h, double* hist) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->in_session && hist, "prcg_get_history: no session or null buffer");
    NOT_RHS2(h, "prcg_get_history");
    int rc = prcg_sync(h);
    if (rc) return rc;
    const int m = h->max_iter;
    std::vector<double> all((size_t)(m + 1) * kNS);
    if ((rc = d2h(h, all.data(), h->dots.d(), (int64_t)(m + 1) * kNS))) return rc;
    static const int slot_of_bit[4] = {PRCG_S_RR, PRCG_S_RES2, PRCG_S_ERRA2, PRCG_S_ERR2};
    int row = 0;
    for (int bit = 0; bit < 4; ++bit) {
        if (!(h->hist_mask & (1u << bit))) continue;
        double* dst = hist + (size_t)row * m;
        for (int k = 0; k < m; ++k)
            dst[k] = k <= h->k ? std::sqrt(all[(size_t)k * kNS + slot_of_bit[bit]]) : 0.0;
        ++row;
    }
    return PRCG_OK;
}

// ---- two or four right-hand sides in one session: Hestenes-Stiefel, predict-and-recompute (PRCG_PR, PRCG_M) ----
int prcg_solve_begin_multi(prcg_t* h, int variant, int nrhs, const double* const* b, const double* const* x0, int max_iter,
                           const double* inv_diag, uint32_t hist_mask) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, nrhs == 2 || nrhs == 4, "prcg_solve_begin_multi: nrhs = %d: the multi-RHS session serves exactly 2 right-hand sides "
                                     "(or 4, as two pairs)", nrhs);
    CHECK(h, variant == PRCG_HS || is_pr(variant), "prcg_solve_begin_multi: variant %d: the two-RHS session serves PRCG_HS (hs_cg / hs_pcg), "
                                                   "PRCG_PR (pr_cg / pr_pcg) and PRCG_M (m_cg / m_pcg) only", variant);
    CHECK(h, !h->multi(), "prcg_solve_begin_multi: a communicator is set on the handle: the two-RHS session runs on one GPU");
    CHECK(h, h->g == 0, "prcg_solve_begin_multi: n_ghost = %lld > 0: the two-RHS session serves whole operators only", (long long)h->g);
    CHECK(h, h->cb == nullptr, "prcg_solve_begin_multi: a host-callback preconditioner is set (prcg_set_preconditioner): the two-RHS "
                               "session serves Jacobi (inv_diag) or none");
    CHECK(h, !h->have_block_jacobi(), "prcg_solve_begin_multi: a block-Jacobi preconditioner is set (prcg_set_block_jacobi): the two-RHS "
                            "session serves Jacobi (inv_diag) or none");
    CHECK(h, h->replace_fn == nullptr, "prcg_solve_begin_multi: a replace hook is set (prcg_set_replace_hook): not served by the two-RHS session");
    CHECK(h, (hist_mask & ~PRCG_HIST_UPDATED_RESIDUAL_2_NORM) == 0,
          "prcg_solve_begin_multi: history bits other than PRCG_HIST_UPDATED_RESIDUAL_2_NORM are not served by the two-RHS session");
    bool have_all = b && x0;
    for (int j = 0; have_all && j < nrhs; ++j) have_all = b[j] && x0[j];
    CHECK(h, have_all, "prcg_solve_begin_multi: null b or x0");
    const int64_t n = h->n, ne = h->n + kGatherPad;
    const size_t D = sizeof(double);
    const int groups = nrhs / 2;
    const bool pr = is_pr(variant);
    // X and P feed the product: like every product source they carry the spare entries behind row n.  The second pair
    // group's arrays (and its block partials) follow the first's, and only a four-RHS session asks for them.
    const size_t src = (size_t)2 * ne * D, vec = (size_t)2 * n * D, tilde = inv_diag ? vec : 16, part = (size_t)8192 * kPartialStride * D;
    int rc;
    if (groups == 1 && !pr)
        rc = open_session(h, "prcg_solve_begin_multi", PRCG_HS, max_iter, hist_mask, inv_diag, false,
                          {{&h->mx, src}, {&h->mp, src}, {&h->mr, vec}, {&h->ms, vec}, {&h->mrt, tilde}});
    else if (groups == 1)
        rc = open_session(h, "prcg_solve_begin_multi", variant, max_iter, hist_mask, inv_diag, false,
                          {{&h->mx, src}, {&h->mp, src}, {&h->mr, vec}, {&h->ms, vec}, {&h->mrt, tilde}, {&h->mst, tilde}}, 2);
    else
        rc = open_session(h, "prcg_solve_begin_multi", variant, max_iter, hist_mask, inv_diag, false,
                          {{&h->mx, src}, {&h->mp, src}, {&h->mr, vec}, {&h->ms, vec}, {&h->mrt, tilde}, {&h->mst, pr ? tilde : 16},
                           {&h->mx1, src}, {&h->mp1, src}, {&h->mr1, vec}, {&h->ms1, vec}, {&h->mrt1, tilde}, {&h->mst1, pr ? tilde : 16},
                           {&h->partA1, part}, {&h->partB1, part}}, (pr ? 2 : 1) * 2);
    if (rc) return rc;
    h->rhs2 = true;
    h->groups = groups;
    h->spmm4 = groups == 2 && spmm4_one_launch(h);
    std::vector<double> pairs;
    try { pairs.resize((size_t)2 * n); } catch (const std::bad_alloc&) { return fail(h, PRCG_ENOMEM, "prcg_solve_begin_multi: host staging"); }
    for (int g = 0; g < groups; ++g) {
        const PairGroup G = pair_group(h, g);
        for (int64_t i = 0; i < n; ++i) { pairs[2 * i] = x0[2 * g][i]; pairs[2 * i + 1] = x0[2 * g + 1][i]; }
        if ((rc = h2d(h, G.x->d(), pairs.data(), 2 * n))) return rc;
        for (int64_t i = 0; i < n; ++i) { pairs[2 * i] = b[2 * g][i]; pairs[2 * i + 1] = b[2 * g + 1][i]; }
        if ((rc = h2d(h, G.r->d(), pairs.data(), 2 * n))) return rc;
    }
    hipStream_t sc = h->sc;
    // r = b - A x0 for every column (hs_cg.py:23): one product of [x0_0 x0_1] (| [x0_2 x0_3]), parked in S
    if (groups == 2) LAUNCHCHK(h, eng_spmm4(h, sc, 0, h->mx.d(), h->mx1.d(), h->ms.d(), h->ms1.d()));
    else LAUNCHCHK(h, eng_spmm2(h, sc, 0, h->mx.d(), h->ms.d(), 3));
    for (int g = 0; g < groups; ++g) {
        const PairGroup G = pair_group(h, g);
        launch_sub(sc, G.r->d(), 1, G.r->d(), 1, G.s->d(), 1, 2 * n);
    }
    if (pr2(h)) {
        int g0[2] = {0, 0};
        for (int g = 0; g < groups; ++g) {
            const PairGroup G = pair_group(h, g);
            g0[g] = launch_pr2_init_dots(sc, pr2_args(h, 0, g));             // (r~ = d r); nu = r~.r, r.r   pr_cg.py:108-109
            LAUNCHCHK(h, g0[g]);
            launch_copy(sc, G.p->d(), 1, h->prec ? G.rt->d() : G.r->d(), 1, 2 * n);   // p = r~ (r)   :110
        }
        if ((rc = pr2_product_and_sums(h, 0, g0))) return rc;                // s = A p, (s~ = d s), mu, dl, gm   :111-116
        HIPCHK(h, hipStreamSynchronize(sc));
        h->in_session = true;
        return PRCG_OK;
    }
    for (int g = 0; g < groups; ++g) {
        const PairGroup G = pair_group(h, g);
        const Hs2Args a = hs2_args(h, 0, g);
        const int g1 = launch_hs2_init_dots(sc, a);                          // (r~ = d r); nu = r.r~, r.r   :25 / :86-88
        LAUNCHCHK(h, g1);
        launch_reduce_final(sc, a.partials, g1, dots_at(h, G.row0), kHs2Nu, kHs2Nu, 4);
        launch_copy(sc, G.p->d(), 1, h->prec ? G.rt->d() : G.r->d(), 1, 2 * n);   // p = r~ (r)   :24 / :87
    }
    if ((rc = hs2_product_and_mu(h, 0))) return rc;                          // s = A p, mu = p.s   :26-27
    HIPCHK(h, hipStreamSynchronize(sc));
    h->in_session = true;
    return PRCG_OK;
}

// ---- two right-hand sides in one pipelined predict-and-recompute session (PRCG_PIPE_PR, PRCG_PIPE_PR_M) ----
int prcg_solve_begin_multi_pipe(prcg_t* h, int variant, int nrhs, const double* const* b, const double* const* x0, int max_iter,
                                const double* inv_diag, uint32_t hist_mask) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, variant != PRCG_PIPE_P && variant != PRCG_PIPE_P_M, "prcg_solve_begin_multi_pipe: variant %d: the stored-w flavours (PRCG_PIPE_P, "
          "PRCG_PIPE_P_M) are not served: the pipelined two-RHS session recomputes w = A r in its four-vector product", variant);
    CHECK(h, pipe_recompute(variant), "prcg_solve_begin_multi_pipe: variant %d: the pipelined two-RHS session serves PRCG_PIPE_PR (pipe_pr_cg / "
                                      "pipe_pr_pcg) and PRCG_PIPE_PR_M (pipe_pr_m_cg / pipe_pr_m_pcg) only", variant);
    CHECK(h, nrhs == 2, "prcg_solve_begin_multi_pipe: nrhs = %d: the pipelined session serves exactly 2 right-hand sides (its product is the "
                        "four-vector one; an eight-vector product does not exist)", nrhs);
    CHECK(h, !h->multi(), "prcg_solve_begin_multi_pipe: a communicator is set on the handle: the two-RHS session runs on one GPU");
    CHECK(h, h->g == 0, "prcg_solve_begin_multi_pipe: n_ghost = %lld > 0: the two-RHS session serves whole operators only", (long long)h->g);
    CHECK(h, h->cb == nullptr, "prcg_solve_begin_multi_pipe: a host-callback preconditioner is set (prcg_set_preconditioner): the two-RHS "
                               "session serves Jacobi (inv_diag) or none");
    CHECK(h, !h->have_block_jacobi(), "prcg_solve_begin_multi_pipe: a block-Jacobi preconditioner is set (prcg_set_block_jacobi): the two-RHS "
                            "session serves Jacobi (inv_diag) or none");
    CHECK(h, h->replace_fn == nullptr, "prcg_solve_begin_multi_pipe: a replace hook is set (prcg_set_replace_hook): not served by the two-RHS session");
    CHECK(h, (hist_mask & ~PRCG_HIST_UPDATED_RESIDUAL_2_NORM) == 0,
          "prcg_solve_begin_multi_pipe: history bits other than PRCG_HIST_UPDATED_RESIDUAL_2_NORM are not served by the two-RHS session");
    CHECK(h, b && x0 && b[0] && b[1] && x0[0] && x0[1], "prcg_solve_begin_multi_pipe: null b or x0");
    const int64_t n = h->n, ne = h->n + kGatherPad;
    const size_t D = sizeof(double);
    // the pair array that feeds the product -- (r,s), with Jacobi (r~,s~) -- carries the spare entries of every product source
    const size_t src = (size_t)2 * ne * D, vec = (size_t)2 * n * D;
    int rc = open_session(h, "prcg_solve_begin_multi_pipe", variant, max_iter, hist_mask, inv_diag, false,
                          {{&h->cxp[0], vec}, {&h->cxp[1], vec}, {&h->crs[0], inv_diag ? vec : src}, {&h->crs[1], inv_diag ? vec : src},
                           {&h->cwu[0], vec}, {&h->cwu[1], vec}, {&h->crst[0], inv_diag ? src : 16}, {&h->crst[1], inv_diag ? src : 16},
                           {&h->b, vec}}, 2);
    if (rc) return rc;
    h->rhs2 = true;
    h->groups = 1;
    h->pipe2 = true;
    h->spmm4 = spmm4_one_launch(h);
    std::vector<double> pairs;
    try { pairs.resize((size_t)2 * n); } catch (const std::bad_alloc&) { return fail(h, PRCG_ENOMEM, "prcg_solve_begin_multi_pipe: host staging"); }
    for (int64_t i = 0; i < n; ++i) { pairs[2 * i] = x0[0][i]; pairs[2 * i + 1] = x0[1][i]; }
    if ((rc = h2d(h, h->tmp_ext.d(), pairs.data(), 2 * n))) return rc;
    for (int64_t i = 0; i < n; ++i) { pairs[2 * i] = b[0][i]; pairs[2 * i + 1] = b[1][i]; }
    if ((rc = h2d(h, h->b.d(), pairs.data(), 2 * n))) return rc;
    hipStream_t sc = h->sc;
    DevBuf* in = h->prec ? h->crst : h->crs;                                  // the product's source pairs
    // r = b - A x0 of both columns: one two-vector product of [x0_0 x0_1]   (pipe_pr_cg.py:22-23)
    LAUNCHCHK(h, eng_spmm2(h, sc, 0, h->tmp_ext.d(), h->t1.d(), 3));
    for (int c = 0; c < 2; ++c) {
        launch_copy(sc, h->cxp[c].d(), 2, h->tmp_ext.d() + c, 2, n);                       // x = x0
        launch_sub(sc, h->crs[c].d(), 2, h->b.d() + c, 2, h->t1.d() + c, 2, n);             // r = b - A x
        if (h->prec) launch_mul(sc, h->crst[c].d(), 2, h->dinv.d(), 1, h->crs[c].d(), 2, n);   // r~ = M^-1 r    :124
        launch_copy(sc, h->cxp[c].d() + 1, 2, in[c].d(), 2, n);                             // p = r (r~)     :24 / :125
    }
    // s = A p: p is r (r~), so the product of the source pairs -- their second halves still zero -- leaves it in w's place
    if ((rc = pipe2_product(h))) return rc;
    for (int c = 0; c < 2; ++c) {
        launch_copy(sc, h->crs[c].d() + 1, 2, h->cwu[c].d(), 2, n);                         // s = A p        :26 / :127
        if (h->prec) launch_mul(sc, h->crst[c].d() + 1, 2, h->dinv.d(), 1, h->crs[c].d() + 1, 2, n);   // s~ = M^-1 s   :128
    }
    // (w, u) = A (r, s) (A (r~, s~)): w = A p again, the bits of `w = s.copy()` (:27 / :129), and u = A w = A s (A s~)   :28 / :131
    if ((rc = pipe2_product(h))) return rc;
    const int grid = launch_pipe2_dots(sc, pipe2_args(h, 0));                               // mu, delta, gamma, nu, r.r   :25-36 / :126-140
    LAUNCHCHK(h, grid);
    pipe2_reduce(h, 0, grid);
    HIPCHK(h, hipStreamSynchronize(sc));
    h->in_session = true;
    return PRCG_OK;
}

// (column j of a four-RHS session: column j % 2 of pair group j / 2 -- per column what a two-RHS session returns)
#define NEED_RHS2(h, name, j)                                                                                        \
    do {                                                                                                              \
        CHECK(h, (h)->in_session && (h)->rhs2, name ": no open two-RHS session (prcg_solve_begin_multi)");             \
        CHECK(h, (j) >= 0 && (j) < 2 * (h)->groups, (h)->groups == 2 ? name ": right-hand side %d out of range (0 .. 3)"  \
                                                                    : name ": right-hand side %d out of range (0, 1)", (int)(j)); \
    } while (0)

int prcg_get_vector_rhs(prcg_t* h, int which, int j, double* out) {
    if (!h) return PRCG_EINVAL;
    NEED_RHS2(h, "prcg_get_vector_rhs", j);
    CHECK(h, out, "prcg_get_vector_rhs: null buffer");
    if (h->pipe2) {
        // column j's pairs: (x,p), (r,s), (w,u) -- w = A r, u = A s as the iteration's product left them -- and with Jacobi (r~,s~)
        const double* src = which == PRCG_VEC_X ? h->cxp[j].d() : which == PRCG_VEC_P ? h->cxp[j].d() + 1 :
                            which == PRCG_VEC_R ? h->crs[j].d() : which == PRCG_VEC_S ? h->crs[j].d() + 1 :
                            which == PRCG_VEC_W ? h->cwu[j].d() : which == PRCG_VEC_U ? h->cwu[j].d() + 1 :
                            (which == PRCG_VEC_RT && h->prec) ? h->crst[j].d() : (which == PRCG_VEC_ST && h->prec) ? h->crst[j].d() + 1 : nullptr;
        CHECK(h, src, "prcg_get_vector_rhs: vector %d is not part of the pipelined two-RHS session (x, r, p, s, w, u; rt, st with Jacobi; "
                      "w~ and u~ are formed in registers and never stored)", which);
        int rc = prcg_sync(h);
        if (rc) return rc;
        launch_copy(h->sc, h->t1.d(), 1, src, 2, h->n);
        return d2h(h, out, h->t1.d(), h->n);
    }
    const PairGroup G = pair_group(h, j / 2);
    const DevBuf* src = which == PRCG_VEC_X ? G.x : which == PRCG_VEC_R ? G.r : which == PRCG_VEC_P ? G.p :
                        which == PRCG_VEC_S ? G.s : (which == PRCG_VEC_RT && h->prec) ? G.rt :
                        (which == PRCG_VEC_ST && h->prec && pr2(h)) ? G.st : nullptr;
    CHECK(h, src, "prcg_get_vector_rhs: vector %d is not part of the two-RHS session (x, r, p, s; rt with Jacobi; st with Jacobi "
                  "in a PRCG_PR / PRCG_M session)", which);
    int rc = prcg_sync(h);
    if (rc) return rc;
    launch_copy(h->sc, h->t1.d(), 1, src->d() + j % 2, 2, h->n);
    return d2h(h, out, h->t1.d(), h->n);
}

int prcg_get_scalars_rhs(prcg_t* h, int k, int j, double* out) {
    if (!h) return PRCG_EINVAL;
    NEED_RHS2(h, "prcg_get_scalars_rhs", j);
    CHECK(h, out && k >= 0 && k <= h->max_iter, "prcg_get_scalars_rhs: bad argument");
    int rc = prcg_sync(h);
    if (rc) return rc;
    double row[kNS];
    const int row0 = pair_group(h, j / 2).row0;
    j %= 2;
    if ((rc = d2h(h, row, dots_at(h, row0 + (two_rows(h) ? 2 * k + j : k)), kNS))) return rc;
    for (int q = 0; q < kNS; ++q) out[q] = 0.0;
    if (two_rows(h)) {
        for (int q = 0; q <= PRCG_S_RR; ++q) out[q] = row[q];         // mu, dl, gm, nu, rr: the column's own row
        return PRCG_OK;
    }
    out[PRCG_S_MU] = row[kHs2Mu + j]; out[PRCG_S_NU] = row[kHs2Nu + 2 * j]; out[PRCG_S_RR] = row[kHs2Rr + 2 * j];
    return PRCG_OK;
}

int prcg_get_coefficients_rhs(prcg_t* h, int k, int j, double* out) {
    if (!h) return PRCG_EINVAL;
    NEED_RHS2(h, "prcg_get_coefficients_rhs", j);
    CHECK(h, out && k >= 1 && k <= h->max_iter, "prcg_get_coefficients_rhs: bad argument");
    int rc = prcg_sync(h);
    if (rc) return rc;
    double row[kCoefStride];
    const int row0 = pair_group(h, j / 2).row0;
    j %= 2;
    if ((rc = d2h(h, row, coef_at(h, row0 + (two_rows(h) ? 2 * k + j : k)), kCoefStride))) return rc;
    if (two_rows(h)) { out[0] = row[0]; out[1] = row[1]; out[2] = row[2]; return PRCG_OK; }     // a, b, the predicted nu
    out[0] = row[2 * j]; out[1] = row[2 * j + 1]; out[2] = 0.0;      // Hestenes-Stiefel predicts no nu
    return PRCG_OK;
}

int prcg_get_history_rhs(prcg_t* h, int j, double* hist) {
    if (!h) return PRCG_EINVAL;
    NEED_RHS2(h, "prcg_get_history_rhs", j);
    CHECK(h, hist, "prcg_get_history_rhs: null buffer");
    int rc = prcg_sync(h);
    if (rc) return rc;
    if (!(h->hist_mask & PRCG_HIST_UPDATED_RESIDUAL_2_NORM)) return PRCG_OK;
    const int m = h->max_iter;
    const int rows = two_rows(h) ? 2 : 1;
    std::vector<double> all((size_t)(m + 1) * rows * kNS);
    if ((rc = d2h(h, all.data(), dots_at(h, pair_group(h, j / 2).row0), (int64_t)(m + 1) * rows * kNS))) return rc;
    j %= 2;
    for (int k = 0; k < m; ++k) {
        const double rr = two_rows(h) ? all[(size_t)(2 * k + j) * kNS + PRCG_S_RR] : all[(size_t)k * kNS + kHs2Rr + 2 * j];
        hist[k] = k <= h->k ? std::sqrt(rr) : 0.0;
    }
    return PRCG_OK;
}

int prcg_set_profiling(prcg_t* h, int stride) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, stride >= 0, "prcg_set_profiling: negative stride");
    h->prof_stride = stride;
    h->n_ev_spmv = h->n_ev_upd = 0;
    return PRCG_OK;
}

int prcg_get_timings(prcg_t* h, prcg_timings* t) {
    if (!h || !t) return PRCG_EINVAL;
    int rc = prcg_sync(h);
    if (rc) return rc;
    memset(t, 0, sizeof *t);
    double s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < h->n_ev_spmv; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->ev_spmv[i].a, h->ev_spmv[i].b) == hipSuccess) s1 += ms;
    }
    for (int i = 0; i < h->n_ev_upd; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->ev_upd[i].a, h->ev_upd[i].b) == hipSuccess) s2 += ms;
    }
    t->spmv_samples = h->n_ev_spmv;
    t->spmv_ms = h->n_ev_spmv ? s1 / h->n_ev_spmv : 0.0;
    t->update_ms = h->n_ev_upd ? s2 / h->n_ev_upd : 0.0;
    t->tot_ms = h->last_tot_ms;
    t->iterations = h->last_iters;
    t->iter_ms = h->last_iters ? h->last_tot_ms / h->last_iters : 0.0;
    return PRCG_OK;
}

int prcg_solve(prcg_t* h, int variant, const double* b, const double* x0, int max_iter, const double* x_true,
               const double* inv_diag, uint32_t hist_mask, double* hist, double* x_out, prcg_timings* t) {
    if (!h) return PRCG_EINVAL;
    int rc = prcg_solve_begin(h, variant, b, x0, max_iter, x_true, inv_diag, hist_mask);
    if (rc) return rc;
    const auto t0 = std::chrono::steady_clock::now();
    if ((rc = prcg_iterate(h, max_iter - 1))) return rc;
    if ((rc = prcg_sync(h))) return rc;
    const auto t1 = std::chrono::steady_clock::now();
    h->last_tot_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    h->last_iters = max_iter - 1;
    if (hist && hist_mask && (rc = prcg_get_history(h, hist))) return rc;
    if (x_out && (rc = prcg_get_vector(h, PRCG_VEC_X, x_out))) return rc;
    if (t) rc = prcg_get_timings(h, t);
    return rc;
}

int64_t prcg_plan_operator(int64_t n_rows, int64_t n_ghost, int64_t nnz, const int32_t* indptr32, const int32_t* indices,
                           const double* data, const char* const* keys, const char* const* values, int n_options, int64_t* out,
                           int64_t capacity) {
    constexpr int64_t kFields = 18;
    if (n_rows < 0 || n_ghost < 0 || nnz < 0 || !indptr32 || (nnz > 0 && (!indices || !data)) || n_options < 0 ||
        (n_options > 0 && (!keys || !values)) || !out)
        return -1;
    if (capacity < kFields) return -kFields;
    if (indptr32[0] != 0 || indptr32[n_rows] != nnz) return -1;
    for (int64_t i = 0; i < n_rows; ++i)
        if (indptr32[i + 1] < indptr32[i]) return -1;
    Options opt;
    for (int i = 0; i < n_options; ++i)
        if (!apply_option(opt, keys[i], values[i])) return -1;
    OperatorPlan pl;
    std::string why;
    if (!plan_operator(opt, n_rows, n_ghost, nnz, indptr32, indices, data, pl, why)) return -1;
    const int cw = pl.win_pat ? 0 : (pl.win_geom < 2 ? 1 : 2);
    out[0] = pl.win ? 1 : (pl.sell ? 2 : 0);
    out[1] = pl.win ? pl.win_geom : -1;
    out[2] = pl.win ? pl.win_rows : 0;
    out[3] = pl.win_pat ? 1 : 0;
    out[4] = pl.sweep_waves;
    out[5] = pl.win ? pl.win_vd : pl.vd_int;
    out[6] = pl.win ? pl.win_vd : pl.vd_bnd;
    out[7] = pl.win ? cw : (pl.sell ? 2 : (pl.c8_int ? 1 : (pl.c16_int ? 2 : 4)));
    out[8] = pl.win ? cw : (pl.sell ? 2 : (pl.c8_bnd ? 1 : (pl.c16_bnd ? 2 : 4)));
    out[9] = pl.steps;
    out[10] = pl.win ? pl.nwt_int : (pl.sell ? pl.nst_int : pl.nt_int);
    out[11] = pl.win ? pl.nwt_bnd : (pl.sell ? pl.nst_bnd : pl.nt_bnd);
    out[12] = pl.win_period;
    out[13] = pl.bytes();
    // what upload_operator copies, array after array (an array that is not uploaded adds nothing)
    const uint64_t seed = 0xcbf29ce484222325ull;
    const bool any_vd = pl.vd_int || pl.vd_bnd, win_vd = pl.win && pl.win_vd;
    uint64_t hi = seed, hv = seed, hd = seed, ht = seed;
    hi = fnv1a(hi, pl.c16); hi = fnv1a(hi, pl.c8); hi = fnv1a(hi, pl.tbase);
    if (pl.win) { hi = fnv1a(hi, pl.wcw16); hi = fnv1a(hi, pl.wcw8); hi = fnv1a(hi, pl.wrel); }
    if (pl.sell) { hi = fnv1a(hi, pl.sp.col); hi = fnv1a(hi, pl.sp.rows); hi = fnv1a(hi, pl.sp.gran); }
    if (any_vd) hv = fnv1a(hv, pl.vidx);
    if (win_vd) hv = fnv1a(hv, pl.wvidx);
    if (any_vd) { hd = fnv1a(hd, pl.vdict); hd = fnv1a(hd, pl.vdesc); }
    if (win_vd) hd = fnv1a(hd, pl.wvdict);
    if (pl.win && pl.win_pat) hd = fnv1a(hd, pl.pats);
    if (pl.sell) hd = fnv1a(hd, pl.sp.val);
    ht = fnv1a(ht, pl.tiles);
    if (pl.win) ht = fnv1a(ht, pl.wtiles);
    if (pl.sell) ht = fnv1a(ht, pl.sslices);
    out[14] = (int64_t)hi; out[15] = (int64_t)hv; out[16] = (int64_t)hd; out[17] = (int64_t)ht;
    return kFields;
}

int prcg_plan_values_route(int64_t n_rows, int64_t n_ghost, int64_t nnz, const int32_t* indptr32, const int32_t* indices,
                           const double* data, const char* const* keys, const char* const* values, int n_options) {
    if (n_rows < 0 || n_ghost < 0 || nnz < 0 || !indptr32 || (nnz > 0 && (!indices || !data)) || n_options < 0 ||
        (n_options > 0 && (!keys || !values)))
        return -1;
    if (indptr32[0] != 0 || indptr32[n_rows] != nnz) return -1;
    for (int64_t i = 0; i < n_rows; ++i)
        if (indptr32[i + 1] < indptr32[i]) return -1;
    Options opt;
    for (int i = 0; i < n_options; ++i)
        if (!apply_option(opt, keys[i], values[i])) return -1;
    OperatorPlan pl;
    std::string why;
    if (!plan_operator(opt, n_rows, n_ghost, nnz, indptr32, indices, data, pl, why)) return -1;
    return values_route(pl);
}

int64_t prcg_plan_tiles(int64_t n, const int32_t* indptr, const uint8_t* row_class, int cap_nnz, int cap_rows,
                        int32_t* tiles_out, int64_t capacity, int64_t* n_class0) {
    if (n < 0 || !indptr || cap_nnz < 1 || cap_rows < 1 || (!tiles_out && capacity > 0)) return -1;
    std::vector<Tile> t0, t1;
    plan_tiles(n, indptr, row_class, cap_nnz, cap_rows, t0, t1);
    const int64_t total = (int64_t)t0.size() + (int64_t)t1.size();
    if (n_class0) *n_class0 = (int64_t)t0.size();
    if (total > capacity) return -total;   // tell the caller how much room is needed
    int64_t o = 0;
    for (const auto& t : t0) { tiles_out[2 * o] = t.row_begin; tiles_out[2 * o + 1] = t.row_end; ++o; }
    for (const auto& t : t1) { tiles_out[2 * o] = t.row_begin; tiles_out[2 * o + 1] = t.row_end; ++o; }
    return total;
}

int64_t prcg_plan_window(int64_t n, int64_t n_cols, const int32_t* indptr, const int32_t* indices, const uint8_t* row_class,
                         int rows_per_tile, int32_t* tiles_out, int64_t capacity, uint16_t* cw_out, int64_t* n_class0,
                         int* most_pages) {
    if (n < 0 || n_cols < n || !indptr || (indptr[n] > 0 && !indices) || (rows_per_tile != 64 && rows_per_tile != 128) ||
        (!tiles_out && capacity > 0))
        return -1;
    WinPlan wp;
    plan_window_tiles(n, n_cols, indptr, indices, row_class, rows_per_tile, kWinCapNnz, win_max_pages(rows_per_tile), wp);
    if (!wp.ok0 || !wp.ok1) return 0;                       // not a window operator
    const int64_t total = (int64_t)wp.t0.size() + (int64_t)wp.t1.size();
    if (n_class0) *n_class0 = (int64_t)wp.t0.size();
    if (most_pages) *most_pages = wp.pages0 > wp.pages1 ? wp.pages0 : wp.pages1;
    if (total > capacity) return -total;
    int64_t o = 0;
    for (const auto* v : {&wp.t0, &wp.t1})
        for (const auto& t : *v) { memcpy(tiles_out + 20 * o, &t, 20 * sizeof(int32_t)); ++o; }
    if (cw_out) memcpy(cw_out, wp.cw.data(), (size_t)indptr[n] * sizeof(uint16_t));
    return total;
}

int64_t prcg_plan_window_patterns(int64_t n, int64_t n_cols, const int32_t* indptr, const int32_t* indices, const double* data,
                                  const uint8_t* row_class, int32_t* tiles_out, int64_t tile_capacity, void* pat_out,
                                  int64_t pat_capacity, uint16_t* masks_out, int64_t mask_capacity, int64_t* counts_out) {
    if (n < 0 || n_cols < n || !indptr || (indptr[n] > 0 && (!indices || !data)) || !counts_out) return -1;
    WinPlan wp;
    plan_window_tiles(n, n_cols, indptr, indices, row_class, 64, kWinCapNnz, kWinPatPages, wp);
    if (!wp.ok0 || !wp.ok1) return 0;
    std::vector<WTile> all(wp.t0);
    all.insert(all.end(), wp.t1.begin(), wp.t1.end());
    std::vector<PatRec> pats;
    std::vector<uint16_t> masks;
    if (!plan_window_patterns(all, indptr, wp.cw.data(), data, pats, masks)) return 0;
    counts_out[0] = (int64_t)all.size(); counts_out[1] = (int64_t)pats.size(); counts_out[2] = (int64_t)masks.size();
    if ((int64_t)all.size() > tile_capacity || (int64_t)pats.size() > pat_capacity || (int64_t)masks.size() > mask_capacity ||
        !tiles_out || !pat_out || !masks_out)
        return -(int64_t)all.size();
    static_assert(sizeof(WTile) == 24 * sizeof(int32_t), "24 int32 per tile");
    memcpy(tiles_out, all.data(), all.size() * sizeof(WTile));
    memcpy(pat_out, pats.data(), pats.size() * sizeof(PatRec));
    memcpy(masks_out, masks.data(), masks.size() * sizeof(uint16_t));
    return 1;
}

int64_t prcg_plan_sweep(int64_t n, const int32_t* indptr, const int32_t* indices, const double* data, int max_waves,
                        int32_t* tiles_out, int64_t tile_capacity, void* pat_out, int64_t pat_capacity, uint16_t* masks_out,
                        int64_t mask_capacity, int64_t* counts_out) {
    if (n < 0 || !indptr || (indptr[n] > 0 && (!indices || !data)) || !counts_out) return -1;
    SweepPlan sw;
    std::vector<PatRec> pats;
    std::vector<uint16_t> masks;
    if (!plan_sweep_tiles(n, n, indptr, indices, kWinPatPages, max_waves, sw)) return 0;
    if (!plan_window_patterns(sw.tiles, indptr, sw.cw.data(), data, pats, masks)) return 0;
    counts_out[0] = (int64_t)sw.tiles.size(); counts_out[1] = (int64_t)pats.size(); counts_out[2] = (int64_t)masks.size();
    counts_out[3] = sw.waves; counts_out[4] = sw.plane; counts_out[5] = sw.rows_per_tile;
    if ((int64_t)sw.tiles.size() > tile_capacity || (int64_t)pats.size() > pat_capacity || (int64_t)masks.size() > mask_capacity ||
        !tiles_out || !pat_out || !masks_out)
        return -(int64_t)sw.tiles.size();
    memcpy(tiles_out, sw.tiles.data(), sw.tiles.size() * sizeof(WTile));
    memcpy(pat_out, pats.data(), pats.size() * sizeof(PatRec));
    memcpy(masks_out, masks.data(), masks.size() * sizeof(uint16_t));
    return 1;
}

int prcg_plan_window_images(int64_t n, int64_t n_cols, const int32_t* indptr, const int32_t* indices, const uint8_t* row_class,
                            int rows_per_tile, int share, int64_t* out) {
    if (n < 0 || n_cols < n || !indptr || (indptr[n] > 0 && !indices) || (rows_per_tile != 64 && rows_per_tile != 128) || !out)
        return -1;
    WinPlan wp;
    plan_window_tiles(n, n_cols, indptr, indices, row_class, rows_per_tile, kWinCapNnz, win_max_pages(rows_per_tile), wp);
    if (!wp.ok0 || !wp.ok1) return 0;
    std::vector<WTile> all(wp.t0);
    all.insert(all.end(), wp.t1.begin(), wp.t1.end());
    std::vector<uint16_t> cstore, rstore;
    std::vector<uint8_t> vstore;
    const StreamStats st = share_window_streams<uint16_t>(all, indptr, wp.cw.data(), nullptr, share != 0, cstore, vstore, rstore);
    // what every tile will read must be what its own image holds
    bool same = true;
    for (const auto& t : all) {
        const int pad = t.lo & 15;
        same = same && (t.src_c & 15) == 0 && (size_t)t.src_c + pad + (t.hi - t.lo) <= cstore.size() &&
               memcmp(cstore.data() + t.src_c + pad, wp.cw.data() + t.lo, (size_t)(t.hi - t.lo) * sizeof(uint16_t)) == 0;
        for (int r = t.rb; r <= t.re && same; ++r) same = rstore[(size_t)t.src_r + (r - t.rb)] == (uint16_t)(indptr[r] - t.lo);
    }
    out[0] = (int64_t)all.size(); out[1] = st.cw_images; out[2] = st.rel_images;
    out[3] = (int64_t)cstore.size(); out[4] = (int64_t)rstore.size(); out[5] = same ? 1 : 0;
    return 1;
}

int64_t prcg_plan_sell(int64_t n, const int32_t* indptr, const int32_t* indices, const double* data, const uint8_t* row_class,
                       double max_overhead, int sigma, int planes, int allow_runs, int window_granules, int32_t* slices_out, int64_t capacity,
                       double* val_out, uint16_t* col_out, int64_t array_capacity, int32_t* rows_out, int64_t rows_capacity,
                       int32_t* gran_out, int64_t gran_capacity, int64_t* stats) {
    if (n < 0 || !indptr || (indptr[n] > 0 && (!indices || !data)) || (!slices_out && capacity > 0)) return -1;
    SellPlan sp;
    SellOptions so;
    so.max_overhead = max_overhead; so.sigma = sigma; so.planes = planes; so.allow_runs = allow_runs != 0;
    so.window_granules = window_granules;
    if (!plan_sell(n, indptr, indices, data, row_class, so, sp)) return 0;
    const int64_t total = (int64_t)sp.s0.size() + (int64_t)sp.s1.size();
    if (stats) {
        stats[0] = (int64_t)sp.s0.size(); stats[1] = (int64_t)sp.val.size(); stats[2] = (int64_t)sp.col.size(); stats[3] = sp.padded_nnz;
        stats[4] = sp.sigma; stats[5] = sp.stride_rows; stats[6] = sp.planes; stats[7] = (int64_t)sp.rows.size();
        stats[8] = sp.col_entries; stats[9] = sp.run; stats[10] = sp.window; stats[11] = (int64_t)sp.gran.size();
    }
    if (total > capacity || (val_out && (int64_t)sp.val.size() > array_capacity) || (col_out && (int64_t)sp.col.size() > array_capacity) ||
        (rows_out && (int64_t)sp.rows.size() > rows_capacity) || (gran_out && (int64_t)sp.gran.size() > gran_capacity)) return -total;
    int64_t o = 0;
    for (const auto* v : {&sp.s0, &sp.s1})
        for (const auto& t : *v) { memcpy(slices_out + 8 * o, &t, 8 * sizeof(int32_t)); ++o; }
    if (val_out) memcpy(val_out, sp.val.data(), sp.val.size() * sizeof(double));
    if (col_out) memcpy(col_out, sp.col.data(), sp.col.size() * sizeof(uint16_t));
    if (rows_out && !sp.rows.empty()) memcpy(rows_out, sp.rows.data(), sp.rows.size() * sizeof(int32_t));
    if (gran_out && !sp.gran.empty()) memcpy(gran_out, sp.gran.data(), sp.gran.size() * sizeof(int32_t));
    return total;
}

int prcg_plan_gather(int rank, int doubles_per_table, const double* tables, int n_peers, const int32_t* peer_rank,
                     const int64_t* recv_ptr, int64_t slot_doubles, int32_t* ghost_src) {
    if (rank < 0 || doubles_per_table < 1 || !tables || n_peers < 0 || slot_doubles < 8 || (slot_doubles & 1)) return -1;
    if (n_peers > 0 && (!peer_rank || !recv_ptr || !ghost_src)) return -1;
    return plan_gather_sources(rank, doubles_per_table, tables, n_peers, peer_rank, recv_ptr, slot_doubles, ghost_src);
}

int64_t prcg_debug_layout(const prcg_t* h, int64_t* out, int64_t capacity) {
    if (!h || !h->have_csr || !out) return -1;
    const int64_t nt = h->win ? (int64_t)h->nwt_int + h->nwt_bnd : (int64_t)h->nt_int + h->nt_bnd;
    const int64_t need = 8 + 2 * nt;
    if (capacity < need) return -need;
    out[0] = h->win ? 1 : 0;
    out[1] = h->win ? h->win_geom : -1;
    out[2] = h->win ? h->win_rows : 0;
    out[3] = nt;
    // the session's last launch that left inner-product partials: its workgroups and, on a window operator, the waves per
    // workgroup it ran with (before any such launch: what the one-launch pipelined iteration would take)
    out[4] = h->last_grid;
    out[5] = !h->win ? 4 : (h->last_grid > 0 ? h->last_wpb
                            : win_fused_waves_per_block(h->win_geom, h->win_vd, h->fused_comm, h->nwt_int + h->nwt_bnd, h->opt.want_big, h->sweep_waves));
    out[6] = h->win ? h->nwt_int : h->nt_int;
    out[7] = h->win ? (int64_t)h->sweep_waves << 8 : 0;    // bit 0: always 0 (was the retired XCD-chunked tile order); >> 8: waves of a sweep table
    std::vector<int32_t> rows((size_t)nt * 2);
    if (h->win) {
        std::vector<WTile> t((size_t)nt);
        if (nt && hipMemcpy(t.data(), h->wtiles.p, (size_t)nt * sizeof(WTile), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        for (int64_t i = 0; i < nt; ++i) { out[8 + 2 * i] = t[(size_t)i].rb; out[9 + 2 * i] = t[(size_t)i].re; }
    } else {
        std::vector<Tile> t((size_t)nt);
        if (nt && hipMemcpy(t.data(), h->tiles.p, (size_t)nt * sizeof(Tile), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        for (int64_t i = 0; i < nt; ++i) { out[8 + 2 * i] = t[(size_t)i].row_begin; out[9 + 2 * i] = t[(size_t)i].row_end; }
    }
    return need;
}

int64_t prcg_debug_slice_rows(const prcg_t* h, int32_t* out, int64_t capacity) {
    if (!h || !h->have_csr) return -1;
    if (!h->sell) return 0;
    const int64_t ns = (int64_t)h->nst_int + h->nst_bnd;
    const int64_t need = 64 * ns;
    if (capacity < need || !out) return -need;
    // both tables as the kernels read them (slice_row): the descriptors, and the (row, length) pairs of the slices that name rows
    std::vector<SellSlice> s((size_t)ns);
    if (ns && hipMemcpy(s.data(), h->sslices.p, (size_t)ns * sizeof(SellSlice), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    const int64_t npairs = (int64_t)(h->srows.bytes / (2 * sizeof(int32_t)));
    std::vector<int32_t> pairs((size_t)npairs * 2);
    if (npairs && hipMemcpy(pairs.data(), h->srows.p, (size_t)npairs * 2 * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    for (int64_t t = 0; t < ns; ++t) {
        const SellSlice& d = s[(size_t)t];
        if (d.rows_off >= 0 && (int64_t)d.rows_off + 64 > npairs) return -1;
        for (int l = 0; l < 64; ++l)
            out[64 * t + l] = d.rows_off < 0 ? (d.rb + l < d.re ? d.rb + l : -1) : pairs[(size_t)2 * (d.rows_off + l)];
    }
    return need;
}

int prcg_window_source_ok(int64_t n_rows, int64_t n_ghost, int components, int64_t bytes_available) {
    if (n_rows < 0 || n_ghost < 0 || components < 1) return 0;
    return bytes_available >= (n_rows + n_ghost + (int64_t)kGatherPad) * components * (int64_t)sizeof(double) ? 1 : 0;
}

void prcg_tile_caps(int* cap_nnz, int* cap_rows) {
    const char* e = getenv("PRCG_TILE_STEPS");
    if (cap_nnz) *cap_nnz = tile_cap_nnz(pick_tile_steps(e ? atoi(e) : 0));
    if (cap_rows) *cap_rows = kTileCapRows;
}

}  // extern "C"

// ---- what a batch of small systems borrows from its handle (prcg_batch.h; the batch itself: prcg_batch.cpp) ----
namespace prcg {

BatchHost batch_host(const prcg_handle* h) { return BatchHost{h->dev, h->sc, h->multi()}; }

int batch_fail(prcg_handle* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return fail(h, code, "%s", buf);
}

}  // namespace prcg
