// Sessions with one right-hand side: prcg_solve_begin, the iteration of every variant family and schedule, what a launch
// leaves pending and how it is flushed, the recorders, the per-column getters and setters, profiling and prcg_solve.
// open_session, which every session type goes through, lives here too.  Built from the services of prcg_engine.cpp
// (prcg_handle.h); sessions with two or four right-hand sides: prcg_multi.cpp.  Host code only.
#include <hip/hip_runtime_api.h>

#include <chrono>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../include/prcg.h"
#include "prcg_handle.h"

using namespace prcg;

namespace {

// the iterate x: second-class citizen of the pair array XP in the pipelined variants
const double* x_ptr(prcg_t* h) { return is_pipe(h->variant) ? h->xp.d() : h->x.d(); }
int x_stride(prcg_t* h) { return is_pipe(h->variant) ? 2 : 1; }

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
        // everything in order on one stream.  A block-Jacobi session with a threshold (kStopBlockJacobi; no other kind comes here):
        // every launch in its stop form on the session's word, which is complete at each kernel boundary.  The reduction sums row k
        // and decides on it (it returns at once if the session stopped earlier); the product and the pair launch of iteration k
        // belong to the state of k, so they are skipped only if the session stopped BEFORE k -- stopped at k, it holds w, u, u~
        // (w~) of k as well.
        const StopAt stop = h->stop_at(k);
        LAUNCHCHK(h, launch_reduce_final(h->sc, h->partA.d(), grid_upd, dots_at(h, k), 0, 0, 5, stop));
        if (profile) prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
        LAUNCHCHK(h, eng_spmm2(h, h->sc, 0, in_ext, h->wu.d(), mask, stop));
        if (profile) prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
        if (h->bj_session) {
            // block Jacobi: both columns of [w u] in one launch that reads every block once
            if (h->bj_var)
                LAUNCHCHK(h, launch_block_jacobi_var_pair(h->sc, h->wt.d(), h->ut.d(), h->wu.d(), h->bjv_plan.ntiles, h->bjv_tiles_d(), h->bjv_code_d(),
                                                          h->bj_blocks.d(), mask, stop));
            else
                LAUNCHCHK(h, launch_block_jacobi_pair(h->sc, h->wt.d(), h->ut.d(), h->wu.d(), h->n, h->bj_bs, h->bj_blocks.d(), mask, stop));
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
        // (nt_bnd counts CSR-adaptive tiles, whatever family runs: the row classes are shared by the three plans, so the sliced and the
        //  window table have boundary units exactly when this one has; eng_spmm2 takes its own family's range from tile_range)
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
    // (the interior launch's shape, for prcg_debug_layout: the boundary launch's replaces it as "the last launch")
    const int int_grid = epi != kEpiNone ? h->last_grid : 0, int_wpb = epi != kEpiNone ? h->last_wpb : 0;
    HIPCHK(h, hipStreamWaitEvent(h->sc, h->e_halo, 0));
    const int g2 = eng_spmv(h, h->sc, 2, x_ext, y, epi, ep_r, ep_d, ep_st, h->partB.d() + (size_t)g1 * kPartialStride);
    LAUNCHCHK(h, g2);
    if (g1 > 0 && g2 > 0) { h->int_grid = int_grid; h->int_wpb = int_wpb; }
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
        // a one-launch session with a threshold: the reduction also DECIDES on the row it sums (the iteration has no later launch
        // whose prologue would), and returns at once if the session has stopped -- its partials are then stale
        launch_reduce_final(h->sc, h->pend_buf, h->pend_parts, dots_at(h, h->pend_k), 0, 0, 5, h->fused ? h->stop_at(h->pend_k) : StopAt{});
        h->pend_parts = 0;
    }
}

// A session with a threshold of any kind, every stream idle (prcg_sync): has the device stopped it?  The words tell, read once.
// prcg_iterate counted and enqueued without knowing: launches k_stop + 1 .. h->k returned at once and wrote nothing.  A newly stopped
// column records where and why; once EVERY column has stopped (a single session has one) the host's picture goes back to iteration
// k_stop, with two columns the later stop -- the iteration count; the input pairs of a one-launch pipelined session, which every
// enqueued launch flipped once on the host only (the parity of the difference says which buffer launch k_stop wrote; the
// one-workgroup solver works in place: no flip); the two direction buffers of a Hestenes-Stiefel session on a window operator,
// flipped in the same way (on other operators and in the one-workgroup solver p is updated in place); and nothing is pending, neither
// partials nor mu (the reduction that would sum them returns at once as well).  The two-kernel schedules (block Jacobi, two
// right-hand sides) flip nothing and leave nothing pending: only the count goes back.  Idempotent: once resolved, nothing more is
// enqueued and prcg_iterate is a no-op.
int resolve_stop(prcg_t* h) {
    if (!h->in_session || !h->stops() || h->stopped()) return PRCG_OK;
    int w[4] = {-1, 0, -1, 0};
    HIPCHK(h, hipMemcpy(w, h->word, sizeof w, hipMemcpyDeviceToHost));
    for (int c = 0; c < h->stop_cols(); ++c)
        if (h->stopped_k[c] < 0 && w[2 * c] >= 0) { h->stopped_k[c] = w[2 * c]; h->stop_status[c] = w[2 * c + 1]; }
    if (!h->stopped()) return PRCG_OK;
    const int k_stop = h->stop_cols() == 2 && h->stopped_k[1] > h->stopped_k[0] ? h->stopped_k[1] : h->stopped_k[0];
    const bool odd = (h->k - k_stop) & 1;
    if (h->fused && !h->small && odd) {       // (the two-kernel schedules flip nothing)
        double* const bufA = h->prec ? h->rst.d() : h->rs.d();
        double* const bufB = h->prec ? h->rst2.d() : h->rs2.d();
        h->rs_cur = (h->rs_cur == bufA) ? bufB : bufA;
    }
    if (h->stop_kind == kStopHs && h->win && !h->small_hs && odd) h->p_cur = (h->p_cur == h->p.d()) ? h->p2.d() : h->p.d();
    h->pend_parts = 0;
    h->hs_pend_mu = 0;
    h->k = k_stop;
    return PRCG_OK;
}

// The session runs the deferred (x,p) store: single GPU, window operator, no recorder that reads x between two launches
// of one prcg_iterate call.  A property of the open session: PRCG_XP_DEFER is fixed once the operator is set
// (prcg_set_option refuses it after prcg_set_csr), and the arrays in memory are current outside prcg_iterate's loop.
bool xp_deferred(const prcg_t* h) {
    const Session& s = *h;
    return h->opt.want_xp_defer && s.in_session && is_pipe(s.variant) && s.fused && !s.fused_comm && !s.small && h->win && !h->multi() &&
           !records_state(s.hist_mask) && !s.stops();      // (with a threshold every launch closes itself: a stop leaves ONE iteration's state)
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
    if (const StopAt stop = h->stop_at(k - 1)) { f.prev.word = stop.word; f.prev.thr = stop.thr; f.prev.word_k = stop.k; }      // the prologue may stop the session at k - 1
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
    // (with a block-Jacobi threshold: update k is skipped if the session stopped at k - 1 or earlier)
    const int grid = launch_pipe_update(h->sc, a, h->stop_at(k));
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
// (a session with a threshold, prcg_set_stop_hs: the reduction also DECIDES on the row it completes -- the iteration has no later launch
//  whose prologue would -- and returns at once if the session has stopped: its partials are then stale)
void hs_flush(prcg_t* h) {
    if (h->hs_pend_mu > 0) {
        launch_reduce_hs_mu(h->sc, h->partB.d(), h->hs_pend_mu, dots_at(h, h->pend_k), h->stop_at(h->pend_k));
        h->hs_pend_mu = 0;
    }
}

// hs_cg.py:54-62 (hs_pcg :116-125) on one GPU without reduction launches.  The two inner products still separate
// the iteration into two phases (that IS Hestenes-Stiefel), but each phase's block partials are summed by every
// workgroup of the NEXT launch (same fixed order everywhere):
//   launch 1  [mu_k1 from the product's partials; a = nu_k1 / mu_k1]  x += a p;  r -= a s;  (r~ = d r);  nu_k partials
//   launch 2  [nu_k from launch 1's partials; b = nu_k / nu_k1]  window operators: p = z + b p_old formed while the
//             input window is staged, s = A p, mu_k partials, p_k written to the other direction buffer;
//             CSR-adaptive tiles: the p update (with that prologue) and the product are two launches.
// A session with a threshold (prcg_set_stop_hs) decides where mu of the previous iteration becomes known: in the prologue of launch 1,
// which applies the rule to row k - 1 = {mu_k1, nu_k1, rr_k1} and may stop the session at k - 1 (k_hs_update_xr_stop), or in the
// reduction that ends the call (hs_flush).  Launch 2 and the product decide nothing (mu_k does not exist before they have run);
// they return at once if the session stopped BEFORE k.  So the product s_k = A p_k of the stop iteration is computed although
// rr_k was known before it: one product per solve, the price of one rule for every session type.
int iterate_hs_fused(prcg_t* h, int k) {
    HsArgs a = hs_args(h, k);
    const bool have_mu = h->hs_pend_mu > 0 && h->pend_k == k - 1;
    if (!have_mu) hs_flush(h);
    bool on = false;
    prof_begin(h, h->ev_upd, h->n_ev_upd, k, on);
    const StopAt stop = h->stop_at(k);
    const int g1 = launch_hs_update_xr(h->sc, a, have_mu ? h->partB.d() : nullptr, have_mu ? h->hs_pend_mu : 0, dots_at(h, k - 1), stop);
    LAUNCHCHK(h, g1);
    prof_end(h, h->ev_upd, h->n_ev_upd, on);
    h->hs_pend_mu = 0;
    int grid = 0;
    on = false;
    if (h->win) {
        FusedPrev hs{};
        hs.prev_partials = h->partA.d(); hs.nprev = g1;
        hs.dots_prev_out = dots_at(h, k); hs.dots_old = dots_at(h, k - 1);
        if (stop) { hs.word = stop.word; hs.word_k = stop.k; }      // (launch B skips, it never decides)
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
        LAUNCHCHK(h, launch_hs_update_p(h->sc, a, h->partA.d(), g1, dots_at(h, k), stop));      // (launch B and the product skip, they never decide)
        prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
        grid = eng_spmv(h, h->sc, 0, h->p_cur, h->s.d(), kEpiDotXY, nullptr, nullptr, nullptr, h->partB.d(), stop);
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
        const int it_grid = h->last_grid, it_wpb = h->last_wpb, it_int_grid = h->int_grid, it_int_wpb = h->int_wpb;
        if ((rc = dist_spmv(h, h->e_ext.d(), h->t1.d(), kEpiDotXY, nullptr, nullptr, nullptr, &grid))) return rc;
        h->last_grid = it_grid; h->last_wpb = it_wpb; h->int_grid = it_int_grid; h->int_wpb = it_int_wpb;
        launch_reduce_final(h->sc, h->partB.d(), grid, dots_at(h, k), 0, PRCG_S_ERRA2, 1);
    }
    return allreduce(h, dots_at(h, k) + PRCG_S_RES2, 3, h->sc);
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

// what the one-workgroup solvers are handed for `iters` iterations from the current one: the caller-order CSR arrays, the state
// of the session's family (Hestenes-Stiefel: x, r, p, s; pipelined: the pairs (x,p), (r,s)) and both histories
SmallArgs small_args(prcg_t* h, int iters) {
    SmallArgs sa{};
    sa.n = (int)h->n; sa.nnz = (int)h->nnz;
    sa.indptr = h->indptr.i(); sa.col = h->col.i(); sa.val = h->val.d();
    if (h->small_hs) { sa.xp = h->x.d(); sa.rs = h->r.d(); sa.hs_p = h->p_cur; sa.hs_s = h->s.d(); }
    else { sa.xp = h->xp.d(); sa.rs = h->rs_cur; }
    sa.dots = h->dots.d(); sa.coef = h->coef.d();
    sa.k0 = h->k; sa.iters = iters; sa.meurant = h->small_hs ? 0 : meurant(h->variant);
    return sa;
}

// ---- the initial state of each family: what prcg_solve_begin runs behind r0's product A x0 (in t1) ----
int begin_pipe(prcg_t* h) {
    const int variant = h->variant;
    const uint32_t hist_mask = h->hist_mask;
    const int64_t n = h->n, ne = h->n + h->g + kGatherPad;
    const size_t D = sizeof(double);
    hipStream_t sc = h->sc;
    double* tmp = h->tmp_ext.d();
    double* t1 = h->t1.d();
    int rc;
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
    // a session with a threshold runs the single-GPU one-launch schedule or the one-workgroup solver (what prcg_solve_begin let
    // through selects it); every launch closes itself (xp_deferred), so a stopped session holds one complete iteration
    // -- or, with blocks (prcg_set_stop_block_jacobi), the stored-tilde two-kernel schedule, whose launches have stop forms of their own
    CHECK(h, !h->stops() || (h->stop_kind == kStopBlockJacobi ? (h->bj_session && !h->fused) : (h->fused && !h->fused_comm)),
          "prcg_solve_begin: a stop threshold is set and the session did not get the one-launch schedule");
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
    // (with a threshold: the rule on row 0 rides on its reduction -- b = A x0 stops the session before its first iteration)
    LAUNCHCHK(h, launch_reduce_final(sc, h->partA.d(), grid, dots_at(h, 0), 0, 0, 5, h->stop_at(0)));
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
    return PRCG_OK;
}

int begin_cg(prcg_t* h) {
    const int variant = h->variant;
    const int64_t n = h->n, ne = h->n + h->g + kGatherPad;
    const size_t D = sizeof(double);
    hipStream_t sc = h->sc;
    double* t1 = h->t1.d();
    int rc;
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
    return PRCG_OK;
}

int begin_hs_pr(prcg_t* h) {
    const int variant = h->variant;
    const uint32_t hist_mask = h->hist_mask;
    const int64_t n = h->n, ne = h->n + h->g + kGatherPad;
    const size_t D = sizeof(double);
    hipStream_t sc = h->sc;
    double* t1 = h->t1.d();
    int rc;
    // HS and non-pipelined PR share the layout x, r, (r~), p(+ghosts), s, (s~)
    HIPCHK(h, h->p.ensure((size_t)ne * D, h->sc));
    h->p_cur = h->p.d();
    h->hs_fused = variant == PRCG_HS && h->opt.want_fused && !h->multi() && h->g == 0 && !h->stored_tilde;
    // one-workgroup solver (k_small_hs): only when nothing but the recurrence residual is recorded
    h->small_hs = h->hs_fused && h->opt.want_small && !h->prec &&
                  !records_state(hist_mask) &&
                  small_fits(h->n, h->nnz, h->max_row_len, &h->small_mode);
    // a session with a threshold (prcg_set_stop_hs) runs the schedule without reduction launches or the one-workgroup solver: what
    // prcg_solve_begin let through selects one of them
    CHECK(h, h->stop_kind != kStopHs || h->hs_fused, "prcg_solve_begin: a Hestenes-Stiefel stop threshold is set and the session did not get the schedule without reduction launches");
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
        // (with a threshold, prcg_set_stop_hs: the rule on row 0 rides on the reduction that completes it -- b = A x0 stops the session
        //  before its first iteration)
        launch_reduce_hs_mu(sc, h->partB.d(), grid, dots_at(h, 0), h->stop_at(0));   // mu = p.s  :27
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
    return PRCG_OK;
}

}  // namespace

namespace prcg {

// ---- session start --------------------------------------------------------------------------------------------
// Every session is opened here, whichever family it belongs to: the shared argument checks, THE reset of the session state
// (the only assignment of Session{}), the fields every family fills the same way, the caller's leading vectors (`lead`:
// allocated before the scalar arrays, as they always were -- the order of hipMalloc decides where a vector lies), then
// dinv, dots and coef, and the profiling sample counts.  The session stays closed (in_session false) until its family
// has computed the initial state.
int open_session(prcg_t* h, const char* who, int variant, int max_iter, uint32_t hist_mask, const double* inv_diag, bool have_xtrue,
                 std::initializer_list<Lead> lead, int rows_per_iteration) {
    return open_session(h, who, variant, max_iter, hist_mask, inv_diag, have_xtrue, lead.begin(), lead.size(), rows_per_iteration);
}
int open_session(prcg_t* h, const char* who, int variant, int max_iter, uint32_t hist_mask, const double* inv_diag, bool have_xtrue,
                 const Lead* lead, size_t count, int rows_per_iteration) {
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
    for (size_t i = 0; i < count; ++i) HIPCHK(h, lead[i].buf->ensure(lead[i].bytes, h->sc));
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

// ---- stop requests: what each begin path does not serve ------------------------------------------------------
int refuse_unserved_stops(prcg_t* h, const char* who, BeginPath path, int variant, const double* inv_diag) {
    const auto set = [h](StopKind kind) { return h->stop_req[kind].set; };
    if (path != kBeginSingle) {
        // the sessions with several right-hand sides: only the pipelined two-RHS one stops, by per-column thresholds; no such
        // session is begun while a threshold it cannot stop by is set (the Hestenes-Stiefel multi-RHS sessions do not stop: a follow-up)
        CHECK(h, !set(kStopRhs) || path == kBeginMultiPipe,
              "%s: per-column stop thresholds are set (prcg_set_stop_rhs), which serve the pipelined two-RHS session only "
              "(prcg_solve_begin_multi_pipe: PRCG_PIPE_PR, PRCG_PIPE_PR_M, Jacobi or none); this session cannot stop -- "
              "prcg_set_stop_rhs(h, 0, NULL) clears the thresholds", who);
        CHECK(h, !set(kStopBlockJacobi),
              "%s: a block-Jacobi stop threshold is set (prcg_set_stop_block_jacobi), which serves pipelined SINGLE sessions with point-block "
              "Jacobi only (prcg_solve_begin); this session cannot stop by it -- prcg_set_stop_block_jacobi(h, NULL) clears the threshold", who);
        CHECK(h, !set(kStopHs),
              "%s: a Hestenes-Stiefel stop threshold is set (prcg_set_stop_hs), which serves SINGLE PRCG_HS sessions only "
              "(prcg_solve_begin); this session cannot stop by it -- prcg_set_stop_hs(h, NULL) clears the threshold", who);
        return PRCG_OK;
    }
    const bool one_gpu = !h->multi() && h->g == 0, stored = !inv_diag && (h->cb || h->have_block_jacobi());
    if (set(kStopPipe)) {
        const char* const served = "a stop threshold is set (prcg_set_stop), which serves the pipelined variants (PRCG_PIPE_PR, PRCG_PIPE_PR_M, PRCG_PIPE_P, "
                                   "PRCG_PIPE_P_M) on one GPU, unpreconditioned or with inv_diag, on the one-launch schedule or the one-workgroup solver";
        CHECK(h, is_pipe(variant), "%s: %s; variant %d is not pipelined (prcg_set_stop(h, NULL) clears the threshold)", who, served, variant);
        CHECK(h, one_gpu, "%s: %s; this handle has a communicator or ghost rows", who, served);
        CHECK(h, !stored, "%s: %s; a host-callback or block-Jacobi preconditioner is in force (the stored-tilde schedule cannot stop)", who, served);
        CHECK(h, h->opt.want_fused, "%s: %s; PRCG_FUSED=0 selects the two-kernel schedule, which cannot stop", who, served);
        CHECK(h, !h->replace_fn, "%s: %s; a replace hook is set", who, served);
    }
    if (set(kStopBlockJacobi)) {
        const char* const served = "a block-Jacobi stop threshold is set (prcg_set_stop_block_jacobi), which serves the pipelined variants (PRCG_PIPE_PR, "
                                   "PRCG_PIPE_PR_M, PRCG_PIPE_P, PRCG_PIPE_P_M) on one GPU with point-block Jacobi in force";
        const char* const clears = "(prcg_set_stop_block_jacobi(h, NULL) clears the threshold)";
        CHECK(h, is_pipe(variant), "%s: %s; variant %d is not pipelined %s", who, served, variant, clears);
        CHECK(h, one_gpu, "%s: %s; this handle has a communicator or ghost rows %s", who, served, clears);
        CHECK(h, !inv_diag, "%s: %s; inv_diag overrides the blocks -- a session with a diagonal stops through prcg_set_stop %s", who, served, clears);
        CHECK(h, !h->cb, "%s: %s; a host-callback preconditioner is in force %s", who, served, clears);
        CHECK(h, h->have_block_jacobi(), "%s: %s; no blocks are in force -- a session without blocks stops through prcg_set_stop %s", who, served, clears);
        CHECK(h, !h->replace_fn, "%s: %s; a replace hook is set %s", who, served, clears);
    }
    if (set(kStopHs)) {
        const char* const served = "a Hestenes-Stiefel stop threshold is set (prcg_set_stop_hs), which serves PRCG_HS on one GPU, unpreconditioned or with inv_diag, "
                                   "on the schedule without reduction launches or the one-workgroup solver";
        const char* const clears = "(prcg_set_stop_hs(h, NULL) clears the threshold)";
        CHECK(h, variant == PRCG_HS, "%s: %s; variant %d is not Hestenes-Stiefel %s", who, served, variant, clears);
        CHECK(h, one_gpu, "%s: %s; this handle has a communicator or ghost rows %s", who, served, clears);
        CHECK(h, !stored, "%s: %s; a host-callback or block-Jacobi preconditioner is in force (the stored-tilde schedule with reduction "
                          "launches cannot stop) %s", who, served, clears);
        CHECK(h, h->opt.want_fused, "%s: %s; PRCG_FUSED=0 selects the schedule with reduction launches, which cannot stop %s", who, served, clears);
        CHECK(h, !h->replace_fn, "%s: %s; a replace hook is set %s", who, served, clears);
    }
    return PRCG_OK;
}

int arm_stop(prcg_t* h, StopKind kind) {
    static const int kRunning[4] = {-1, 0, -1, 0};
    if (!h->stop_words.p) HIPCHK(h, h->stop_words.alloc(sizeof kRunning));
    HIPCHK(h, hipMemcpyAsync(h->stop_words.p, kRunning, sizeof kRunning, hipMemcpyHostToDevice, h->sc));
    h->stop_kind = kind;
    h->thr[0] = h->stop_req[kind].thr[0]; h->thr[1] = h->stop_req[kind].thr[1];
    h->word = h->stop_words.i();
    return PRCG_OK;
}

}  // namespace prcg

namespace {

// prcg_set_stop, prcg_set_stop_block_jacobi, prcg_set_stop_hs (`name`): the request of `kind` set to *rr_stop or, with NULL, cleared
int set_stop_request(prcg_t* h, StopKind kind, const char* name, const double* rr_stop) {
    if (!h) return PRCG_EINVAL;
    if (!rr_stop) { h->stop_req[kind] = Handle::StopRequest{}; return PRCG_OK; }
    CHECK(h, std::isfinite(*rr_stop) && *rr_stop >= 0.0, "%s: rr_stop = %g: the threshold must be finite and >= 0 (r.r <= rr_stop stops "
                                                         "the session; NULL clears it)", name, *rr_stop);
    h->stop_req[kind].set = true; h->stop_req[kind].thr[0] = *rr_stop;
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
    // a threshold is set: only sessions that can stop on the device are begun -- nothing falls back
    if (int rc = refuse_unserved_stops(h, "prcg_solve_begin", kBeginSingle, variant, inv_diag)) return rc;
    // every vector that feeds a matrix product has ghost room AND kGatherPad spare entries: the
    // narrow column encodings decode a few out-of-tile bytes per tile against the tile's own base
    // (products nobody reads); the pad keeps those gathers inside the allocation without a test
    const int64_t n = h->n, ne = h->n + h->g + kGatherPad;
    const size_t D = sizeof(double);
    int rc = open_session(h, "prcg_solve_begin", variant, max_iter, hist_mask, inv_diag, x_true != nullptr,
                          {{&h->x, (size_t)n * D}, {&h->b, (size_t)n * D}, {&h->xt, (size_t)n * D}, {&h->e_ext, (size_t)ne * D}});
    if (rc) return rc;
    // (what refuse_unserved_stops let through is at most one request: each serves what the others refuse)
    for (const StopKind kind : {kStopPipe, kStopBlockJacobi, kStopHs})
        if (h->stop_req[kind].set && (rc = arm_stop(h, kind))) return rc;
    if ((rc = h2d(h, h->x.d(), x0, n))) return rc;
    if ((rc = h2d(h, h->b.d(), b, n))) return rc;
    if (x_true && (rc = h2d(h, h->xt.d(), x_true, n))) return rc;
    hipStream_t sc = h->sc;
    double* tmp = h->tmp_ext.d();
    double* t1 = h->t1.d();

    // r0 = b - A x0   (hs_cg.py:23, pipe_pr_cg.py:23)
    launch_copy(sc, tmp, 1, h->x.d(), 1, n);
    if ((rc = dist_spmv(h, tmp, t1, kEpiNone, nullptr, nullptr, nullptr, nullptr))) return rc;

    if ((rc = is_pipe(variant) ? begin_pipe(h) : is_cg_family(variant) ? begin_cg(h) : begin_hs_pr(h))) return rc;
    if ((rc = record(h, 0))) return rc;
    HIPCHK(h, hipStreamSynchronize(sc));
    h->in_session = true;
    return PRCG_OK;
}

int prcg_iterate(prcg_t* h, int iters) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->in_session, "prcg_iterate: no open session");
    CHECK(h, iters >= 0, "prcg_iterate: negative count");
    if (h->stopped()) return PRCG_OK;            // stopped at its threshold, every column at its own (prcg_sync has seen the words): a no-op
    CHECK(h, h->k + iters <= h->max_iter, "prcg_iterate: %d more iterations exceed max_iter=%d (k=%d)", iters,
          h->max_iter, h->k);
    HIPCHK(h, hipSetDevice(h->dev));
    if (h->fused_comm && *h->err_host != 0u)
        return fail(h, PRCG_ERCCL, "a one-launch iteration waited more than its bound for the other ranks (a peer stalled or died); "
                                   "the session's results are invalid -- PRCG_PEER=0 / PRCG_FUSED_COMM=0 select the two-kernel schedule");
    if (h->rhs2) {
        for (int i = 0; i < iters; ++i) {
            if (const int rc = iterate_multi(h, h->k + 1)) return rc;
            ++h->k;
        }
        return PRCG_OK;
    }
    if ((h->small_hs || h->small) && iters > 0) {
        // all `iters` iterations inside one launch of one workgroup (Hestenes-Stiefel or pipelined)
        if (h->small_hs) hs_flush(h);
        const SmallArgs sa = small_args(h, iters);
        const StopAt stop = h->stop_at(h->k);
        const SmallStop ss = stop.decides();
        bool on = false;
        prof_begin(h, h->ev_spmv, h->n_ev_spmv, 0, on);
        LAUNCHCHK(h, h->small_hs ? launch_small_hs(h->sc, sa, h->small_mode, stop ? &ss : nullptr) : launch_small_pipe_pr(h->sc, sa, h->small_mode, stop ? &ss : nullptr));
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
    return resolve_stop(h);
}

int prcg_set_stop(prcg_t* h, const double* rr_stop) { return set_stop_request(h, kStopPipe, "prcg_set_stop", rr_stop); }
int prcg_set_stop_block_jacobi(prcg_t* h, const double* rr_stop) { return set_stop_request(h, kStopBlockJacobi, "prcg_set_stop_block_jacobi", rr_stop); }
int prcg_set_stop_hs(prcg_t* h, const double* rr_stop) { return set_stop_request(h, kStopHs, "prcg_set_stop_hs", rr_stop); }

int prcg_get_stop(prcg_t* h, int32_t* k_stop, int32_t* status) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->in_session, "prcg_get_stop: no open session");
    NOT_RHS2(h, "prcg_get_stop");
    CHECK(h, k_stop && status, "prcg_get_stop: null buffer");
    int rc = prcg_sync(h);
    if (rc) return rc;
    *k_stop = h->stopped_k[0]; *status = h->stopped_k[0] >= 0 ? h->stop_status[0] : 0;
    return PRCG_OK;
}

int prcg_iteration(const prcg_t* h) { return h ? h->k : -1; }

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
    CHECK(h, !h->stops(), "prcg_set_iteration: the open session was begun with a stop threshold (prcg_set_stop, prcg_set_stop_block_jacobi, prcg_set_stop_hs): its state is not set from outside");
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
    CHECK(h, !h->stops(), "prcg_set_vector: the open session was begun with a stop threshold (prcg_set_stop, prcg_set_stop_block_jacobi, prcg_set_stop_hs): its state is not set from outside");
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
    if (h->stopped_k[0] >= 0 && k > h->stopped_k[0]) { memset(out, 0, kNS * sizeof(double)); return PRCG_OK; }      // beyond the stop: not part of the run
    return d2h(h, out, dots_at(h, k), kNS);
}

int prcg_set_scalars(prcg_t* h, int k, const double* in) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->in_session && in && k >= 0 && k <= h->max_iter, "prcg_set_scalars: bad argument");
    NOT_RHS2(h, "prcg_set_scalars");
    CHECK(h, !h->stops(), "prcg_set_scalars: the open session was begun with a stop threshold (prcg_set_stop, prcg_set_stop_block_jacobi, prcg_set_stop_hs): its state is not set from outside");
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
    if (h->stopped_k[0] >= 0 && k > h->stopped_k[0]) { memset(out, 0, 3 * sizeof(double)); return PRCG_OK; }
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

}  // extern "C"
