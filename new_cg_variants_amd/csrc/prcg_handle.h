// The handle behind prcg_t and what the host files of libprcg.so share around it.  Internal: not installed, nothing under
// include/ names it.  Included by prcg_engine.cpp (handle lifetime, operator, communicator, the product services),
// prcg_session.cpp (single-RHS sessions), prcg_multi.cpp (two and four right-hand sides) and prcg_batch.cpp (batches of small
// systems).  What several files use has external linkage in namespace prcg; what one file uses stays in that file's anonymous
// namespace.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

#include "../../include/prcg.h"
#include "prcg_kernels.h"
#include "prcg_bjvar.h"
#include "prcg_plan.h"
#include "prcg_rccl.h"

namespace prcg {

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

// How a session stops at a residual threshold, decided on the device.  A kind names both the request on the handle (its setter:
// Handle::stop_req) and what the session begun from it runs (Session::stop_kind):
//   kStopPipe         prcg_set_stop: a pipelined single session on the one-launch schedule (the prologue of launch k + 1 decides on
//                     row k) or the one-workgroup solver
//   kStopRhs          prcg_set_stop_rhs: the pipelined two-RHS session, each column at its own threshold (two stop words)
//   kStopBlockJacobi  prcg_set_stop_block_jacobi: a pipelined single session with blocks, the stored-tilde two-kernel schedule, every
//                     launch of an iteration in its stop form; fused is off, nothing is ever pending
//   kStopHs           prcg_set_stop_hs: a Hestenes-Stiefel single session on the schedule without reduction launches
//                     (iterate_hs_fused), every launch in its stop form, or the one-workgroup solver's
// (in the order the begin paths consult the requests: refuse_unserved_stops)
enum StopKind { kStopNone = -1, kStopPipe = 0, kStopRhs, kStopBlockJacobi, kStopHs, kNumStopKinds };

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
                                 // complete two-RHS state of its own -- Handle::grp)
    bool spmm4 = false;          // ... two groups: the product of an iteration is ONE four-vector launch (sliced rows, PRCG_SPMM4)
    bool pipe2 = false;          // session type "pipelined predict-and-recompute, two right-hand sides" (prcg_solve_begin_multi_pipe):
                                 // rhs2 with one group, variant PRCG_PIPE_PR / PRCG_PIPE_PR_M, per column the pair arrays cxp, crs, cwu
                                 // (crst) around ONE product of four vectors (spmm4: in one launch); two scalar / coefficient rows per iteration
    int bj_tiles = 0;            // two or four right-hand sides with block Jacobi (prcg_solve_begin_multi_block_jacobi: rhs2 && bj_session): the
                                 // tiles of a block launch = the partial rows each of Handle::bjpart holds
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
    int int_grid = 0;            // that launch was the BOUNDARY half of a product in two launches (overlapped_spmv with a communicator):
    int int_wpb = 0;             // ... workgroups and waves per workgroup of the interior half, whose partial rows come first (else 0)
    // ---- stopped at a residual threshold, decided on the device (arm_stop sets these; one set for every kind, sized for two columns) ----
    StopKind stop_kind = kStopNone;      // how the session stops (kStopNone: it was begun without a threshold) ...
    double thr[2] = {0.0, 0.0};          // ... at this threshold on r.r (kStopRhs: column c's; else [0])
    int* word = nullptr;                 // ... through these stop words in device memory (Handle::stop_words), column c's at word + 2 c: {-1, 0}
                                         // while it runs, {k_stop, status} once a launch's prologue, a deciding reduction or the one-workgroup
                                         // solver has stopped it
    int stopped_k[2] = {-1, -1};         // what prcg_sync has read from the words: the iteration whose state column c holds (-1: running) ...
    int stop_status[2] = {0, 0};         // ... and why (1 converged, 2 breakdown)
    bool stops() const { return stop_kind != kStopNone; }
    int stop_cols() const { return stop_kind == kStopRhs ? 2 : 1; }
    bool column_stopped(int c) const { return stops() && c < stop_cols() && stopped_k[c] >= 0; }
    bool stopped() const { return column_stopped(0) && (stop_cols() == 1 || column_stopped(1)); }      // every column: prcg_iterate is a no-op
    // how iteration k (of column c) stops: what every launcher of the iteration takes last -- none for a session without a threshold
    StopAt stop_at(int k, int c = 0) const { return stops() ? StopAt{thr[c], word + 2 * c, k} : StopAt{}; }
};

// One PAIR GROUP of a session with two or four right-hand sides: the interleaved n x 2 arrays X, R, P, S, RT of two columns
// (Hs2Args, prcg_kernels.h) and, for predict-and-recompute with Jacobi, ST (Pr2Args)
struct PairBufs { DevBuf x, r, p, s, rt, st; };

// a vector open_session allocates before the scalar arrays, and its size
struct Lead { DevBuf* buf; size_t bytes; };

// The resident operator (Operator) and the state of the open session (Session) are base sub-objects, so that each is a
// value of its own -- the operator's flags are assigned from the plan, the session is reset as a whole -- while the code
// below addresses their fields as before.
struct Handle : Operator, Session {
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
    PairBufs grp[2];             // two right-hand sides: grp[0]; four: grp[1] is the SECOND pair group (columns 2, 3).  Hestenes-Stiefel: dots /
                                 // coef hold both columns per row; predict-and-recompute: one row per column and iteration
    DevBuf partA1, partB1;       // ... the second group's block partials (the first group's: partA / partB)
    DevBuf bjpart[2][2];         // ... with block Jacobi: the partial rows of group g's block launches (k_block_jacobi_dots: one per TILE, about
                                 // n / 255 -- more than partA's 8192 at large n), column c in bjpart[g][c] (Hestenes-Stiefel: both in [g][0])
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
    // residual thresholds for sessions begun from now on, one request per kind (its setter's), independent of each other: with
    // several set, each begin path refuses by the first it does not serve (refuse_unserved_stops).  thr[1]: kStopRhs only
    struct StopRequest { bool set = false; double thr[2] = {0.0, 0.0}; };
    StopRequest stop_req[kNumStopKinds];
    // the words a session with a threshold stops itself through: four ints, column c's {k, status} at 2 c (SmallStop's layout),
    // allocated once, armed to {-1, 0} when a session of any kind begins (arm_stop)
    DevBuf stop_words;
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
                               &st, &st2, &b, &xt, &dinv, &e_ext, &w, &w2, &u, &u2, &tvec, &t2, &ut, &cb_stage, &q, &q2, &grp[0].x, &grp[0].p, &grp[1].x, &grp[1].p, &x4b,
                               &crs[0], &crs[1], &crst[0], &crst[1]};
        const char* c = static_cast<const char*>(ptr);
        for (const DevBuf* d : all)
            if (d->p && c >= static_cast<const char*>(d->p) && c < static_cast<const char*>(d->p) + d->bytes) return d;
        return nullptr;
    }
};

}  // namespace prcg

// prcg_t (include/prcg.h) is this type; its members are prcg::Handle's, declared where the names of namespace prcg are in scope
struct prcg_handle : prcg::Handle {};

namespace prcg {

// sets the text prcg_last_error returns (h == nullptr: the text of errors with no handle) and returns `code`
int fail(prcg_t* h, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));

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

// every source vector of a launch lies in an allocation that holds what the launch may touch, else an error text (prcg_engine.cpp)
int check_sources(prcg_t* h, std::initializer_list<std::pair<const void*, int>> srcs);
#define SRCCHK(h, ...) do { if (check_sources(h, {__VA_ARGS__})) return -2; } while (0)              // inside a launch helper (returns a grid)
#define SRCCHK2(h, ...) do { if (check_sources(h, {__VA_ARGS__})) return PRCG_EINVAL; } while (0)   // inside an iterate_* function

inline bool is_pipe(int v) { return v == PRCG_PIPE_PR || v == PRCG_PIPE_P || v == PRCG_PIPE_PR_M || v == PRCG_PIPE_P_M; }
inline bool is_pr(int v) { return v == PRCG_PR || v == PRCG_M; }
inline bool is_cg_family(int v) { return v == PRCG_CG_CG || v == PRCG_GV; }
inline bool pipe_recompute(int v) { return v == PRCG_PIPE_PR || v == PRCG_PIPE_PR_M; }
inline bool meurant(int v) { return v == PRCG_PIPE_PR_M || v == PRCG_PIPE_P_M || v == PRCG_M; }
// a recorder reads the state vectors after every iteration (so no schedule may leave them stale between two launches)
inline bool records_state(uint32_t hist_mask) {
    return (hist_mask & (PRCG_HIST_RESIDUAL_2_NORM | PRCG_HIST_ERROR_A_NORM | PRCG_HIST_ERROR_2_NORM)) != 0;
}

inline double* dots_at(prcg_t* h, int k) { return h->dots.d() + (size_t)k * kNS; }
inline double* coef_at(prcg_t* h, int k) { return h->coef.d() + (size_t)k * kCoefStride; }

// ---- prcg_engine.cpp: the services every session type is built from ----
// the matrix products (which: 0 = every tile, 1 = interior tiles, 2 = tiles touching ghosts); they return the grid, -2 when refused
// stop (Session::stop_at; none: the launches of a session without a threshold): the product of iteration stop.k in its stop form
// (ProductStop, prcg_kernels.h) -- it skips if the session (the column) stopped BEFORE stop.k and decides nothing
//   eng_spmv   kEpiDotXY on sliced rows or CSR-adaptive tiles only: a Hestenes-Stiefel session that stops (a window operator runs
//              launch_win_hs: -1 here, as for any other epilogue)
//   eng_spmm2  the two-vector product with its write mask
//   eng_spmm4  stop.word is column 0's, column 1's follows it (word + 2): each two-vector launch skips by its own column's word, the
//              one four-vector launch only when both columns stopped before stop.k
int eng_spmv(prcg_t* h, hipStream_t st, int which, const double* x, double* y, SpmvEpilogue epi, const double* ep_r,
             const double* ep_d, double* ep_st, double* partials, const StopAt& stop = StopAt{});
int eng_spmm2(prcg_t* h, hipStream_t st, int which, const double* rs, double* wu, int mask, const StopAt& stop = StopAt{});
bool spmm4_one_launch(const prcg_t* h);
int eng_spmm4(prcg_t* h, hipStream_t st, int which, const double* src0, const double* src1, double* dst0, double* dst1,
              const StopAt& stop = StopAt{});
int eng_fused(prcg_t* h, hipStream_t st, const FusedState& f, int which = 0);
void note_partials_launch(prcg_t* h, int grid);
int exchange(prcg_t* h, double* vec_ext, int nc, hipStream_t st);
int allreduce(prcg_t* h, double* buf, int count, hipStream_t st);
int plan_gather(prcg_t* h);
int dist_spmv(prcg_t* h, double* x_ext, double* y, SpmvEpilogue epi, const double* ep_r, const double* ep_d, double* ep_st, int* grid_out);
void prof_begin(prcg_t* h, std::vector<EventPair>& evs, int& count, int k, bool& on, int shift = 0);
void prof_end(prcg_t* h, std::vector<EventPair>& evs, int& count, bool on);
int h2d(prcg_t* h, double* dst, const double* src, int64_t count);
int d2h(prcg_t* h, double* dst, const double* src, int64_t count);
// two host columns of n entries, `stride` doubles apart, <-> one interleaved n x 2 pair array on the device (who: the entry's name)
int upload_pairs(prcg_t* h, const char* who, double* dst, const double* col0, const double* col1, int stride = 1);
int download_pairs(prcg_t* h, const char* who, const double* src, double* col0, double* col1, int stride = 1);
int apply_prec(prcg_t* h, const double* src, int sstride, double* dst, int dstride);
int place_session_vectors(prcg_t* h, size_t xp_bytes, size_t rs_bytes);

// ---- prcg_session.cpp: every session, whichever file begins it, is opened here ----
int open_session(prcg_t* h, const char* who, int variant, int max_iter, uint32_t hist_mask, const double* inv_diag, bool have_xtrue,
                 std::initializer_list<Lead> lead, int rows_per_iteration = 1);
// ... with a list made at run time (prcg_multi.cpp: open_pairs).  Hidden: the library exports the symbols it always did
__attribute__((visibility("hidden")))
int open_session(prcg_t* h, const char* who, int variant, int max_iter, uint32_t hist_mask, const double* inv_diag, bool have_xtrue,
                 const Lead* lead, size_t count, int rows_per_iteration);

// ... and so is every stop request consulted and every stop word armed.  "A request of kind K is set: does this begin path serve
// it?" -- the requests in the order of StopKind, the first unserved one refuses in the name of the entry (who); a path consults only
// the kinds it always did (the multi-RHS entries pass prcg_set_stop's by, prcg_solve_begin passes prcg_set_stop_rhs's by)
enum BeginPath { kBeginSingle, kBeginMulti, kBeginMultiPipe };      // (kBeginMulti: prcg_solve_begin_multi and _multi_block_jacobi)
int refuse_unserved_stops(prcg_t* h, const char* who, BeginPath path, int variant = -1, const double* inv_diag = nullptr);
// the session just opened stops by the handle's request of `kind`: its thresholds copied, its words armed to "running" on the
// compute stream (before the first deciding launch is enqueued)
int arm_stop(prcg_t* h, StopKind kind);

// ---- prcg_multi.cpp: iteration k of the open session with two or four right-hand sides (Session::rhs2) ----
int iterate_multi(prcg_t* h, int k);

}  // namespace prcg
