// libprcg.so engine: handle lifetime and options, preconditioner setters, communicator / halo / peer setup, operator upload
// (planned in prcg_plan.cpp), and the services the sessions are built from -- matrix products, halo exchange, all-reduce,
// M^-1, host <-> device copies (declared in prcg_handle.h).  The sessions themselves: prcg_session.cpp (one right-hand
// side), prcg_multi.cpp (two and four), prcg_batch.cpp (batches of small systems).  Implements include/prcg.h.  Host code
// only; kernels live in the .hip files.
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
#include "prcg_handle.h"
#include "prcg_bjvar.h"
#include "prcg_plan.h"
#include "prcg_rccl.h"

using namespace prcg;

namespace {

std::string g_last_error;   // errors with no handle to hang them on

}  // namespace

namespace prcg {

int fail(prcg_t* h, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_last_error = buf;
    return code;
}

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

namespace {

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

}  // namespace

// The launch that left inner-product partials last -- what prcg_debug_layout reports: on a window operator the workgroups and
// waves per workgroup launch_win_v used (win_last_launch: call this right behind the launch), else the grid alone.
void note_partials_launch(prcg_t* h, int grid) {
    if (grid <= 0) return;
    const WinLaunchShape s = h->win ? win_last_launch() : WinLaunchShape{grid, 0};
    h->last_grid = s.grid; h->last_wpb = s.wpb;
    h->int_grid = 0; h->int_wpb = 0;         // (one launch over its tiles, until overlapped_spmv says otherwise)
}
int eng_spmv(prcg_t* h, hipStream_t st, int which, const double* x, double* y, SpmvEpilogue epi, const double* ep_r,
             const double* ep_d, double* ep_st, double* partials, const StopAt& stop) {
    SRCCHK(h, {x, 1});
    const TileRange t = tile_range(h, which);
    if (h->win) {
        if (stop) return -1;      // (the window kernels have no stop form of this product: launch_win_hs serves such a session)
        const int grid = launch_win_spmv(st, h->wdev(), h->wtile_ptr(t.first), t.count, h->win_geom, x, y, epi, ep_r, ep_d, ep_st, partials,
                                         h->opt.win_per_cu);
        if (epi != kEpiNone) note_partials_launch(h, grid);
        return grid;
    }
    const int grid = h->sell
        ? launch_sell_spmv(st, h->sdev(), h->sslice_ptr(t.first), t.count, x, y, epi, ep_r, ep_d, ep_st, partials, h->opt.sell_per_cu, stop)
        : launch_spmv(st, csr_view(h, which), h->tile_ptr(t.first), t.count, h->steps, x, y, epi, ep_r, ep_d, ep_st, partials, h->opt.kn, stop);
    if (epi != kEpiNone) note_partials_launch(h, grid);
    return grid;
}
int eng_spmm2(prcg_t* h, hipStream_t st, int which, const double* rs, double* wu, int mask, const StopAt& stop) {
    SRCCHK(h, {rs, 2});
    const TileRange t = tile_range(h, which);
    if (h->win) return launch_win_spmm2(st, h->wdev(), h->wtile_ptr(t.first), t.count, h->win_geom, rs, wu, mask, h->opt.win_per_cu, stop);
    if (h->sell) return launch_sell_spmm2(st, h->sdev(), h->sslice_ptr(t.first), t.count, rs, wu, mask, h->opt.sell_per_cu, stop);
    return launch_spmm2(st, csr_view(h, which), h->tile_ptr(t.first), t.count, h->steps, rs, wu, mask, h->opt.kn, stop);
}
// [dst0 | dst1] = A [src0 | src1], two pair arrays: one launch on sliced rows (PRCG_SPMM4=0: never), else a two-vector
// product per pair -- the same bits per column either way
bool spmm4_one_launch(const prcg_t* h) { return h->sell && h->opt.want_spmm4; }
int eng_spmm4(prcg_t* h, hipStream_t st, int which, const double* src0, const double* src1, double* dst0, double* dst1, const StopAt& stop) {
    SRCCHK(h, {src0, 2}, {src1, 2});
    if (spmm4_one_launch(h)) {
        const TileRange t = tile_range(h, which);
        return launch_sell_spmm4(st, h->sdev(), h->sslice_ptr(t.first), t.count, src0, src1, dst0, dst1, h->opt.sell_per_cu, stop);
    }
    const int g0 = eng_spmm2(h, st, which, src0, dst0, 3, stop);
    if (g0 < 0) return g0;
    // (column 1 skips by its own word, which follows column 0's)
    return eng_spmm2(h, st, which, src1, dst1, 3, stop ? StopAt{stop.thr, stop.word + 2, stop.k} : stop);
}
// (only the window kernels have the deferred form that runs one class of tiles; the others always take every tile)
int eng_fused(prcg_t* h, hipStream_t st, const FusedState& f, int which) {
    SRCCHK(h, {f.in_old, 2});
    const TileRange t = tile_range(h, h->win ? which : 0);
    if (h->win)
        return launch_win_pipe_fused(st, h->wdev(), h->wtile_ptr(t.first), t.count, h->win_geom, f,
                                     f.deferred ? h->opt.defer_per_cu : h->opt.win_per_cu);
    if (h->sell) return launch_sell_pipe_fused(st, h->sdev(), h->sslice_ptr(t.first), t.count, f, h->opt.sell_per_cu);
    return launch_pipe_fused(st, h->csr(), h->tile_ptr(t.first), t.count, h->steps, f, h->opt.kn);
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

// `shift`: sample iteration k when k - shift is a multiple of the stride (see iterate_pipe_fused)
void prof_begin(prcg_t* h, std::vector<EventPair>& evs, int& count, int k, bool& on, int shift) {
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

// Two host columns of n entries <-> one interleaved n x 2 pair array on the device, through a host staging vector.  The
// columns' entries lie `stride` doubles apart (1: two vectors; 4: two columns of an n x 4 array); who names the entry.
int upload_pairs(prcg_t* h, const char* who, double* dst, const double* col0, const double* col1, int stride) {
    const int64_t n = h->n;
    std::vector<double> pairs;
    try { pairs.resize((size_t)2 * n); } catch (const std::bad_alloc&) { return fail(h, PRCG_ENOMEM, "%s: host staging", who); }
    for (int64_t i = 0; i < n; ++i) { pairs[2 * i] = col0[i * stride]; pairs[2 * i + 1] = col1[i * stride]; }
    return h2d(h, dst, pairs.data(), 2 * n);
}
int download_pairs(prcg_t* h, const char* who, const double* src, double* col0, double* col1, int stride) {
    const int64_t n = h->n;
    std::vector<double> pairs;
    try { pairs.resize((size_t)2 * n); } catch (const std::bad_alloc&) { return fail(h, PRCG_ENOMEM, "%s: host staging", who); }
    if (int rc = d2h(h, pairs.data(), src, 2 * n)) return rc;
    for (int64_t i = 0; i < n; ++i) { col0[i * stride] = pairs[2 * i]; col1[i * stride] = pairs[2 * i + 1]; }
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

}  // namespace prcg

namespace {

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
    int rc;
    for (int g = 0; g < 2; ++g)
        if ((rc = upload_pairs(h, "prcg_spmm4", g == 0 ? h->tmp_ext.d() : h->x4b.d(), x4 + 2 * g, x4 + 2 * g + 1, 4))) return rc;
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
    for (int g = 0; g < 2; ++g)
        if ((rc = download_pairs(h, "prcg_spmm4", g == 0 ? h->t1.d() : h->y4b.d(), y4 + 2 * g, y4 + 2 * g + 1, 4))) return rc;
    return PRCG_OK;
}

int64_t prcg_operator_bytes(const prcg_t* h) { return (h && h->have_csr) ? h->bytes() : -1; }

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
    const int64_t need = 10 + 2 * nt;
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
    // a product with a dot epilogue in TWO launches (a communicator session's overlapped product): out[4], out[5] are the boundary
    // launch's, these the interior launch's, whose partial rows lie first -- 0, 0: the last launch ran over all the tiles
    out[8] = h->int_grid;
    out[9] = h->int_wpb;
    if (h->win) {
        std::vector<WTile> t((size_t)nt);
        if (nt && hipMemcpy(t.data(), h->wtiles.p, (size_t)nt * sizeof(WTile), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        for (int64_t i = 0; i < nt; ++i) { out[10 + 2 * i] = t[(size_t)i].rb; out[11 + 2 * i] = t[(size_t)i].re; }
    } else {
        std::vector<Tile> t((size_t)nt);
        if (nt && hipMemcpy(t.data(), h->tiles.p, (size_t)nt * sizeof(Tile), hipMemcpyDeviceToHost) != hipSuccess) return -1;
        for (int64_t i = 0; i < nt; ++i) { out[10 + 2 * i] = t[(size_t)i].row_begin; out[11 + 2 * i] = t[(size_t)i].row_end; }
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

int64_t prcg_debug_interior_slices(const prcg_t* h) {
    if (!h || !h->have_csr) return -1;
    return h->sell ? h->nst_int : 0;
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
