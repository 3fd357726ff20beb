// Sessions with two or four right-hand sides: prcg_solve_begin_multi (Hestenes-Stiefel, predict-and-recompute),
// prcg_solve_begin_multi_pipe (pipelined predict-and-recompute), prcg_solve_begin_multi_block_jacobi (Hestenes-Stiefel and
// predict-and-recompute preconditioned by the handle's point-block Jacobi), their iterations (iterate_multi, called by prcg_iterate)
// and the per-column getters.  The first and the last entry are their argument checks around open_pairs and start_pairs, the
// ONE way a session of pair groups is opened and started; with blocks the iterations branch at one step (h->bj_session).  The
// pipelined session has a state layout of its own.  Built from the services of prcg_engine.cpp and open_session
// (prcg_handle.h); the kernels: prcg_rhs2.hip, prcg_blockjac.hip.  Host code only.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <vector>

#include "../../include/prcg.h"
#include "prcg_handle.h"

using namespace prcg;

namespace {

// Two right-hand sides in one Hestenes-Stiefel session (hs_cg.py:54-62 / hs_pcg :116-125 for each column): the vector
// kernels of prcg_rhs2.hip around ONE two-vector product of [p_0 p_1] -- the operator is streamed once for both systems.
// Four right-hand sides are two PAIR GROUPS, each a complete state of this kind (its own arrays, block partials and rows of
// dots / coef: group g's rows follow group g - 1's max_iter + 1 iterations), around ONE product of both groups' directions.
bool pr2(const prcg_t* h) { return h->rhs2 && is_pr(h->variant); }
// the session keeps one scalar and one coefficient row per column and iteration, each in the single-session order
bool two_rows(const prcg_t* h) { return pr2(h) || h->pipe2; }
// pair group g (Handle::grp[g]): its first row of dots / coef ...
int row0(const prcg_t* h, int g) { return g * (h->max_iter + 1) * (pr2(h) ? 2 : 1); }
// ... and its block partials: the first group's are the handle's, the second group has its own
double* part_a(prcg_t* h, int g) { return (g == 0 ? h->partA : h->partA1).d(); }
double* part_b(prcg_t* h, int g) { return (g == 0 ? h->partB : h->partB1).d(); }
// s = A p of every column: one two-vector product, or with two pair groups one product of [P_0 P_1 | P_2 P_3]
int multi_product(prcg_t* h, int k) {
    PairBufs* G = h->grp;
    bool on = false;
    prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
    if (h->groups == 2) LAUNCHCHK(h, eng_spmm4(h, h->sc, 0, G[0].p.d(), G[1].p.d(), G[0].s.d(), G[1].s.d()));
    else LAUNCHCHK(h, eng_spmm2(h, h->sc, 0, G[0].p.d(), G[0].s.d(), 3));
    prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
    return PRCG_OK;
}

// ---- the same sessions preconditioned by the handle's point-block Jacobi (prcg_solve_begin_multi_block_jacobi: h->bj_session) ----
// The state and the scalar rows are those above; r~ (and s~) are stored vectors, and M^-1 is ONE launch per group that
// applies the blocks to both columns and leaves, in the same launch, the partials of the inner products that need the result
// (prcg_blockjac.hip: k_block_jacobi_dots / k_block_jacobi_var_dots) -- one partial row per tile in the session's own arrays.
// The iterations below branch on h->bj_session at the one step that differs:
//   Hestenes-Stiefel: update_xr (unpreconditioned: x, r) -> block NU (r~ = M^-1 r; nu, rr) -> reduce -> update_p -> product ->
//                     dot_ps -> reduce                                                           (hs_cg.py:116-125 per column)
//   PR / M:           update (r~ -= a s~ from the stored vectors) -> product -> block PR (s~ = M^-1 s; mu, dl, gm) -> ONE
//                     reduction launch for both columns' five sums                               (pr_cg.py:146-158 per column)
double* bj_part(prcg_t* h, int g, int c) { return h->bjpart[g][c].d(); }
// the tiles of a block launch with the blocks on the handle = the partial rows a session allocates (0: the blocks give none)
int64_t bj_tile_count(const prcg_t* h) { return h->bj_var ? h->bjv_plan.ntiles : block_jacobi_tiles(h->n, h->bj_bs); }
// one block launch of group g; the grid is checked against the partial rows the session allocated BEFORE anything is launched
int bj2_launch(prcg_t* h, int mode, int g, bool two_arrays, const double* v, double* z) {
    const PairBufs& G = h->grp[g];
    const int64_t tiles = bj_tile_count(h);
    const size_t need = (size_t)tiles * kPartialStride * sizeof(double);
    CHECK(h, tiles > 0 && tiles == h->bj_tiles && h->bjpart[g][0].bytes >= need && (!two_arrays || h->bjpart[g][1].bytes >= need),
          "block-Jacobi multi-RHS session: a block launch of %lld tiles does not match the %d partial rows the session allocated",
          (long long)tiles, h->bj_tiles);
    BjDotsArgs a{};
    a.n = h->n; a.v = v; a.z = z; a.p = G.p.d(); a.r = G.r.d();
    a.part0 = bj_part(h, g, 0); a.part1 = two_arrays ? bj_part(h, g, 1) : nullptr;
    const int grid = h->bj_var ? launch_block_jacobi_var_dots(h->sc, mode, a, tiles, h->bjv_tiles_d(), h->bjv_code_d(), h->bj_blocks.d())
                               : launch_block_jacobi_dots(h->sc, mode, a, h->bj_bs, h->bj_blocks.d());
    LAUNCHCHK(h, grid);
    CHECK(h, grid == h->bj_tiles, "block-Jacobi multi-RHS session: a block launch ran %d workgroups, the session allocated %d partial rows",
          grid, h->bj_tiles);
    return PRCG_OK;
}
// Hestenes-Stiefel: r~ = M^-1 r, nu_c, rr_c of group g -> scalar row k
int bj2_hs_nu(prcg_t* h, int k, int g) {
    const PairBufs& G = h->grp[g];
    if (int rc = bj2_launch(h, kBjDotsNu, g, false, G.r.d(), G.rt.d())) return rc;
    ReduceJobs J{};                                             // (the final tree with a thread's loads batched: one row per tile)
    J.job[0] = ReduceJob{bj_part(h, g, 0), h->bj_tiles, dots_at(h, row0(h, g) + k), kHs2Nu, kHs2Nu, 4};            // nu_0, rr_0, nu_1, rr_1
    launch_reduce_final_jobs(h->sc, J, 1);
    return PRCG_OK;
}

Hs2Args hs2_args(prcg_t* h, int k, int g) {
    const PairBufs& G = h->grp[g];
    Hs2Args a{};
    a.n = h->n;
    a.x = G.x.d(); a.r = G.r.d(); a.rt = h->prec ? G.rt.d() : nullptr; a.p = G.p.d(); a.s = G.s.d();
    a.d = (h->prec && !h->bj_session) ? h->dinv.d() : nullptr;      // (block Jacobi: r~ is a stored vector, no diagonal)
    a.dots_prev = k > 0 ? dots_at(h, row0(h, g) + k - 1) : nullptr;
    a.dots_cur = dots_at(h, row0(h, g) + k);
    a.coef_out = coef_at(h, row0(h, g) + k);
    a.partials = part_a(h, g);
    return a;
}
// s = A p for every column, then per group mu_c = p.s (a launch of its own: the multi-vector products have no dot epilogue)
int hs2_product_and_mu(prcg_t* h, int k) {
    int rc = multi_product(h, k);
    if (rc) return rc;
    for (int g = 0; g < h->groups; ++g) {
        Hs2Args a = hs2_args(h, k, g);
        a.partials = part_b(h, g);
        const int grid = launch_hs2_dot_ps(h->sc, a);
        LAUNCHCHK(h, grid);
        launch_reduce_final(h->sc, a.partials, grid, dots_at(h, row0(h, g) + k), kHs2Mu, kHs2Mu, 2);
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
        // nu_0, rr_0, nu_1, rr_1.  Blocks: a.d is null, so the update moved x and r only (its own partials of r.r stay unused) and
        // the block launch leaves r~ and the sums; else the update's partials hold them
        if (h->bj_session) { if (int rc = bj2_hs_nu(h, k, g)) return rc; }
        else launch_reduce_final(h->sc, a.partials, g1, dots_at(h, row0(h, g) + k), kHs2Nu, kHs2Nu, 4);
        LAUNCHCHK(h, launch_hs2_update_p(h->sc, a));            // p = r~ + b p
    }
    return hs2_product_and_mu(h, k);
}

// Two right-hand sides in one predict-and-recompute session (pr_cg.py:146-158 for each column; PRCG_M: Meurant's prediction):
// update, ONE two-vector product of [p_0 p_1], the three inner products that need s, one reduction launch per column.
Pr2Args pr2_args(prcg_t* h, int k, int g) {
    const PairBufs& G = h->grp[g];
    Pr2Args a{};
    a.n = h->n;
    a.x = G.x.d(); a.r = G.r.d(); a.p = G.p.d(); a.s = G.s.d();
    a.rt = h->prec ? G.rt.d() : nullptr; a.st = h->prec ? G.st.d() : nullptr;
    a.d = (h->prec && !h->bj_session) ? h->dinv.d() : nullptr;      // (block Jacobi: r~, s~ are stored vectors, no diagonal)
    a.dots_prev = k > 0 ? dots_at(h, row0(h, g) + 2 * (k - 1)) : nullptr;   // rows 2 (k - 1), 2 (k - 1) + 1: the columns' sums of k - 1
    a.coef_out = coef_at(h, row0(h, g) + 2 * k);
    a.part0 = part_a(h, g); a.part1 = part_b(h, g);
    a.meurant = meurant(h->variant);
    return a;
}
// Blocks.  Per group s~ = M^-1 s with mu, dl, gm; then the five sums of each column in one reduction launch: mu, dl, gm from the
// tile partials, nu, rr from the update launch's (g_upd[g] blocks) -- at the start (g_upd null) from the tile partials too (block NU)
int bj2_pr_sums(prcg_t* h, int k, int g, const int* g_upd) {
    const PairBufs& G = h->grp[g];
    if (int rc = bj2_launch(h, kBjDotsPr, g, true, G.s.d(), G.st.d())) return rc;
    const int row = row0(h, g) + 2 * k;
    ReduceJobs J{};
    int nj = 0;
    for (int c = 0; c < 2; ++c) {
        if (g_upd) {
            J.job[nj++] = ReduceJob{bj_part(h, g, c), h->bj_tiles, dots_at(h, row + c), kPr2Mu, kPr2Mu, 3};
            J.job[nj++] = ReduceJob{c == 0 ? part_a(h, g) : part_b(h, g), g_upd[g], dots_at(h, row + c), kPr2Nu, kPr2Nu, 2};
        } else {
            J.job[nj++] = ReduceJob{bj_part(h, g, c), h->bj_tiles, dots_at(h, row + c), 0, 0, 5};
        }
    }
    launch_reduce_final_jobs(h->sc, J, nj);
    return PRCG_OK;
}
// s = A p for every column, (s~ = d s), mu, dl, gm; then the five sums of each column: rows 2 k and 2 k + 1 of its group
// (g_upd[g]: the grid of group g's update launch, whose partials the sums include)
int pr2_product_and_sums(prcg_t* h, int k, const int* g_upd) {
    int rc = multi_product(h, k);
    if (rc) return rc;
    for (int g = 0; g < h->groups; ++g) {
        if (h->bj_session) {
            if ((rc = bj2_pr_sums(h, k, g, g_upd))) return rc;
            continue;
        }
        const Pr2Args a = pr2_args(h, k, g);
        const int grid = launch_pr2_dots(h->sc, a);
        LAUNCHCHK(h, grid);
        CHECK(h, grid == g_upd[g], "two-RHS session: the update and the dots launch disagree on the grid (%d, %d)", g_upd[g], grid);
        const int row = row0(h, g) + 2 * k;
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
        // (blocks: r~ -= a s~ from the stored vectors, no diagonal)
        g_upd[g] = h->bj_session ? launch_pr2_update_stored(h->sc, a) : launch_pr2_update(h->sc, a);
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
// Each column stopped at its own threshold (prcg_set_stop_rhs; Session::stop_kind == kStopRhs).  Column c's stop word -- {iteration, status},
// {-1, 0} while it runs -- is written by the reduction that sums its row k: the stop form of the final reduction applies the
// rule of prcg_set_stop to {mu, nu, rr} of that row and, once the word is set, returns at once.  Every later launch reads the
// words: the update skips a frozen column (no load, no store, no coefficient row, no partial row), the product of iteration k
// skips a column that stopped BEFORE k (the product of iteration k_c belongs to the state of k_c and has run).  So a column
// stopped at k_c holds the complete state of k_c, scalar rows 0 .. k_c and coefficient rows 1 .. k_c, and the other column
// executes what it executes in a session without thresholds.  The host enqueues without knowing; prcg_sync reads the words.
// the five sums of each column from the block partials an update (or dots) launch of `grid` blocks left: rows 2 k, 2 k + 1
int pipe2_reduce(prcg_t* h, int k, int grid) {
    LAUNCHCHK(h, launch_reduce_final(h->sc, h->partA.d(), grid, dots_at(h, 2 * k), 0, 0, 5, h->stop_at(k, 0)));
    LAUNCHCHK(h, launch_reduce_final(h->sc, h->partB.d(), grid, dots_at(h, 2 * k + 1), 0, 0, 5, h->stop_at(k, 1)));
    return PRCG_OK;
}
// (w_c, u_c) = A (r_c, s_c) of both columns (Jacobi: A (r~_c, s~_c)): one launch on sliced rows, else two two-vector launches.
// k > 0 in a session with thresholds: the product of iteration k in its stop form (the start-up products, k = 0, are plain)
int pipe2_product(prcg_t* h, int k = 0) {
    DevBuf* src = h->prec ? h->crst : h->crs;
    LAUNCHCHK(h, eng_spmm4(h, h->sc, 0, src[0].d(), src[1].d(), h->cwu[0].d(), h->cwu[1].d(), k > 0 ? h->stop_at(k) : StopAt{}));
    return PRCG_OK;
}
int iterate_pipe2(prcg_t* h, int k) {
    const Pipe2Args a = pipe2_args(h, k);
    bool on = false;
    prof_begin(h, h->ev_upd, h->n_ev_upd, k, on);
    const int grid = launch_pipe2_update(h->sc, a, h->stop_at(k));
    LAUNCHCHK(h, grid);
    prof_end(h, h->ev_upd, h->n_ev_upd, on);
    if (const int rc = pipe2_reduce(h, k, grid)) return rc;
    prof_begin(h, h->ev_spmv, h->n_ev_spmv, k, on);
    const int rc = pipe2_product(h, k);
    if (rc) return rc;
    prof_end(h, h->ev_spmv, h->n_ev_spmv, on);
    return PRCG_OK;
}

// What no session with several right-hand sides serves, refused in the name of the entry that was called (who) and of its
// session (noun: "two-RHS" / "multi-RHS").  Two halves, because the block-Jacobi entry tests its variant and nrhs between them.
// The handle: one GPU, a whole operator, and the preconditioner -- blocks wanted (the block-Jacobi entry) or refused
int refuse_handle(prcg_t* h, const char* who, const char* noun, bool want_blocks) {
    CHECK(h, !h->multi(), "%s: a communicator is set on the handle: the %s session runs on one GPU", who, noun);
    CHECK(h, h->g == 0, "%s: n_ghost = %lld > 0: the %s session serves whole operators only", who, (long long)h->g, noun);
    if (want_blocks) {
        CHECK(h, h->have_block_jacobi(), "%s: no block-Jacobi preconditioner is set on the handle (prcg_set_block_jacobi, prcg_build_block_jacobi, "
                                         "prcg_set_block_jacobi_var, prcg_build_block_jacobi_var; prcg_set_csr drops the blocks): without blocks "
                                         "the session is prcg_solve_begin_multi", who);
        return PRCG_OK;
    }
    CHECK(h, h->cb == nullptr, "%s: a host-callback preconditioner is set (prcg_set_preconditioner): the %s "
                               "session serves Jacobi (inv_diag) or none", who, noun);
    CHECK(h, !h->have_block_jacobi(), "%s: a block-Jacobi preconditioner is set (prcg_set_block_jacobi): the %s "
                            "session serves Jacobi (inv_diag) or none", who, noun);
    return PRCG_OK;
}
// ... the replace hook and the histories
int refuse_hooks(prcg_t* h, const char* who, const char* noun, uint32_t hist_mask) {
    CHECK(h, h->replace_fn == nullptr, "%s: a replace hook is set (prcg_set_replace_hook): not served by the %s session", who, noun);
    CHECK(h, (hist_mask & ~PRCG_HIST_UPDATED_RESIDUAL_2_NORM) == 0,
          "%s: history bits other than PRCG_HIST_UPDATED_RESIDUAL_2_NORM are not served by the %s session", who, noun);
    return PRCG_OK;
}
int refuse_unserved(prcg_t* h, const char* who, uint32_t hist_mask) {
    if (int rc = refuse_handle(h, who, "two-RHS", false)) return rc;
    return refuse_hooks(h, who, "two-RHS", hist_mask);
}
// every b[j] and x0[j] of the nrhs columns is there
bool have_columns(const double* const* b, const double* const* x0, int nrhs) {
    bool all = b && x0;
    for (int j = 0; all && j < nrhs; ++j) all = b[j] && x0[j];
    return all;
}

// ---- one way to open and start a session of pair groups (prcg_solve_begin_multi, prcg_solve_begin_multi_block_jacobi) ----
// The leading vectors of `groups` pair groups, in THE order every such session has allocated them (open_session: the order of
// hipMalloc decides where a vector lies): per group x, p (product sources: the spare entries behind row n), r, s, r~, s~; the
// second group's block partials of its update launch; with blocks (tiles > 0) one partial row per tile of a block launch, per
// group and column.  r~ is a full vector with Jacobi or blocks, s~ in a PR / M session with either; what is not kept is 16 bytes.
int open_pairs(prcg_t* h, const char* who, int variant, int groups, int max_iter, uint32_t hist_mask, const double* inv_diag, int64_t tiles) {
    const size_t D = sizeof(double);
    const bool pr = is_pr(variant);
    const size_t src = (size_t)2 * (h->n + kGatherPad) * D, vec = (size_t)2 * h->n * D, tilde = (inv_diag || tiles) ? vec : 16,
                 part = (size_t)8192 * kPartialStride * D, bjp = (size_t)tiles * kPartialStride * D;
    Lead lead[18];
    size_t count = 0;
    for (int g = 0; g < groups; ++g) {
        for (const Lead& l : {Lead{&h->grp[g].x, src}, Lead{&h->grp[g].p, src}, Lead{&h->grp[g].r, vec}, Lead{&h->grp[g].s, vec},
                              Lead{&h->grp[g].rt, tilde}})
            lead[count++] = l;
        // (the one session that never asked for an s~ it does not keep: Hestenes-Stiefel, one group, no blocks -- it still does not,
        //  so that it allocates and clears exactly what it did)
        if (pr || groups == 2 || tiles) lead[count++] = Lead{&h->grp[g].st, pr ? tilde : 16};
    }
    if (groups == 2) { lead[count++] = Lead{&h->partA1, part}; lead[count++] = Lead{&h->partB1, part}; }
    for (int g = 0; tiles && g < groups; ++g) { lead[count++] = Lead{&h->bjpart[g][0], bjp}; lead[count++] = Lead{&h->bjpart[g][1], pr ? bjp : 16}; }
    return open_session(h, who, variant, max_iter, hist_mask, inv_diag, false, lead, count, (pr ? 2 : 1) * groups);
}
// The start of the session open_pairs opened: X0 and B per group, r = b - A x0, per group r~ / nu / rr and p = r~, the first
// product and its sums -- Jacobi or none through the init kernels of prcg_rhs2.hip, blocks through the block launches.
int start_pairs(prcg_t* h, const char* who, int groups, const double* const* b, const double* const* x0, int64_t tiles) {
    PairBufs* const G = h->grp;
    const int64_t n = h->n;
    hipStream_t sc = h->sc;
    int rc;
    h->rhs2 = true;
    h->groups = groups;
    h->spmm4 = groups == 2 && spmm4_one_launch(h);
    h->bj_tiles = (int)tiles;
    for (int g = 0; g < groups; ++g) {
        if ((rc = upload_pairs(h, who, G[g].x.d(), x0[2 * g], x0[2 * g + 1]))) return rc;
        if ((rc = upload_pairs(h, who, G[g].r.d(), b[2 * g], b[2 * g + 1]))) return rc;
    }
    // r = b - A x0 for every column (hs_cg.py:23): one product of [x0_0 x0_1] (| [x0_2 x0_3]), parked in S
    if (groups == 2) LAUNCHCHK(h, eng_spmm4(h, sc, 0, G[0].x.d(), G[1].x.d(), G[0].s.d(), G[1].s.d()));
    else LAUNCHCHK(h, eng_spmm2(h, sc, 0, G[0].x.d(), G[0].s.d(), 3));
    for (int g = 0; g < groups; ++g) launch_sub(sc, G[g].r.d(), 1, G[g].r.d(), 1, G[g].s.d(), 1, 2 * n);
    int g0[2] = {0, 0};                                  // PR / M with Jacobi or none: the grids of the init launches, whose partials hold nu, rr
    for (int g = 0; g < groups; ++g) {
        // (r~ = M^-1 r); nu = r~.r, r.r   (hs_cg.py:25 / :86-88, pr_cg.py:107-109)
        if (h->bj_session) {
            if ((rc = pr2(h) ? bj2_launch(h, kBjDotsNu, g, true, G[g].r.d(), G[g].rt.d()) : bj2_hs_nu(h, 0, g))) return rc;
        } else if (pr2(h)) {
            g0[g] = launch_pr2_init_dots(sc, pr2_args(h, 0, g));
            LAUNCHCHK(h, g0[g]);
        } else {
            const Hs2Args a = hs2_args(h, 0, g);
            const int g1 = launch_hs2_init_dots(sc, a);
            LAUNCHCHK(h, g1);
            launch_reduce_final(sc, a.partials, g1, dots_at(h, row0(h, g)), kHs2Nu, kHs2Nu, 4);
        }
        launch_copy(sc, G[g].p.d(), 1, h->prec ? G[g].rt.d() : G[g].r.d(), 1, 2 * n);   // p = r~ (r)   hs_cg.py:24 / :87, pr_cg.py:110
    }
    // s = A p; Hestenes-Stiefel: mu = p.s (:26-27); PR / M: (s~ = M^-1 s), mu, dl, gm and the five sums of row 0 (pr_cg.py:111-116)
    if ((rc = pr2(h) ? pr2_product_and_sums(h, 0, h->bj_session ? nullptr : g0) : hs2_product_and_mu(h, 0))) return rc;
    HIPCHK(h, hipStreamSynchronize(sc));
    h->in_session = true;
    return PRCG_OK;
}

}  // namespace

int prcg::iterate_multi(prcg_t* h, int k) { return h->pipe2 ? iterate_pipe2(h, k) : pr2(h) ? iterate_pr2(h, k) : iterate_hs2(h, k); }

extern "C" {

// ---- two or four right-hand sides in one session: Hestenes-Stiefel, predict-and-recompute (PRCG_PR, PRCG_M) ----
int prcg_solve_begin_multi(prcg_t* h, int variant, int nrhs, const double* const* b, const double* const* x0, int max_iter,
                           const double* inv_diag, uint32_t hist_mask) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, nrhs == 2 || nrhs == 4, "prcg_solve_begin_multi: nrhs = %d: the multi-RHS session serves exactly 2 right-hand sides "
                                     "(or 4, as two pairs)", nrhs);
    CHECK(h, variant == PRCG_HS || is_pr(variant), "prcg_solve_begin_multi: variant %d: the two-RHS session serves PRCG_HS (hs_cg / hs_pcg), "
                                                   "PRCG_PR (pr_cg / pr_pcg) and PRCG_M (m_cg / m_pcg) only", variant);
    if (int rc = refuse_unserved(h, "prcg_solve_begin_multi", hist_mask)) return rc;
    if (int rc = refuse_unserved_stops(h, "prcg_solve_begin_multi", kBeginMulti)) return rc;
    CHECK(h, have_columns(b, x0, nrhs), "prcg_solve_begin_multi: null b or x0");
    if (int rc = open_pairs(h, "prcg_solve_begin_multi", variant, nrhs / 2, max_iter, hist_mask, inv_diag, 0)) return rc;
    return start_pairs(h, "prcg_solve_begin_multi", nrhs / 2, b, x0, 0);
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
    if (int rc = refuse_unserved(h, "prcg_solve_begin_multi_pipe", hist_mask)) return rc;
    if (int rc = refuse_unserved_stops(h, "prcg_solve_begin_multi_pipe", kBeginMultiPipe)) return rc;
    CHECK(h, have_columns(b, x0, 2), "prcg_solve_begin_multi_pipe: null b or x0");
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
    // per-column thresholds (prcg_set_stop_rhs): copied now, the words armed to "running" before the first reduction is enqueued
    if (h->stop_req[kStopRhs].set && (rc = arm_stop(h, kStopRhs))) return rc;
    if ((rc = upload_pairs(h, "prcg_solve_begin_multi_pipe", h->tmp_ext.d(), x0[0], x0[1]))) return rc;
    if ((rc = upload_pairs(h, "prcg_solve_begin_multi_pipe", h->b.d(), b[0], b[1]))) return rc;
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
    if ((rc = pipe2_reduce(h, 0, grid))) return rc;
    HIPCHK(h, hipStreamSynchronize(sc));
    h->in_session = true;
    return PRCG_OK;
}

// ---- two or four right-hand sides preconditioned by the point-block Jacobi in force on the handle ----
int prcg_solve_begin_multi_block_jacobi(prcg_t* h, int variant, int nrhs, const double* const* b, const double* const* x0, int max_iter,
                                        uint32_t hist_mask) {
    if (!h) return PRCG_EINVAL;
    const char* const who = "prcg_solve_begin_multi_block_jacobi";
    CHECK(h, h->have_csr, "%s: call prcg_set_csr first", who);
    // (a handle with a communicator cannot hold blocks at all: those two refusals come first so that each names its own reason)
    if (int rc = refuse_handle(h, who, "multi-RHS", true)) return rc;
    CHECK(h, !is_pipe(variant), "%s: variant %d: the pipelined variants are not served with blocks (a follow-up: their session is "
                                "prcg_solve_begin_multi_pipe, Jacobi or none); PRCG_HS, PRCG_PR and PRCG_M are", who, variant);
    CHECK(h, variant == PRCG_HS || is_pr(variant), "%s: variant %d: the block-Jacobi multi-RHS session serves PRCG_HS (hs_pcg), PRCG_PR (pr_pcg) "
                                                   "and PRCG_M (m_pcg) only", who, variant);
    CHECK(h, nrhs == 2 || nrhs == 4, "%s: nrhs = %d: the session serves exactly 2 right-hand sides (or 4, as two pairs)", who, nrhs);
    if (int rc = refuse_hooks(h, who, "multi-RHS", hist_mask)) return rc;
    if (int rc = refuse_unserved_stops(h, who, kBeginMulti)) return rc;
    CHECK(h, have_columns(b, x0, nrhs), "%s: null b or x0", who);
    CHECK(h, max_iter >= 1, "%s: max_iter must be >= 1", who);
    const int64_t tiles = bj_tile_count(h);
    CHECK(h, tiles > 0 && tiles <= INT32_MAX, "%s: the blocks on the handle give %lld tiles", who, (long long)tiles);
    if (int rc = open_pairs(h, who, variant, nrhs / 2, max_iter, hist_mask, nullptr, tiles)) return rc;
    CHECK(h, h->bj_session, "%s: the session did not open with the handle's blocks", who);
    return start_pairs(h, who, nrhs / 2, b, x0, tiles);
}

// (column j of a four-RHS session: column j % 2 of pair group j / 2 -- per column what a two-RHS session returns)
#define NEED_RHS2(h, name, j)                                                                                        \
    do {                                                                                                              \
        CHECK(h, (h)->in_session && (h)->rhs2, name ": no open two-RHS session (prcg_solve_begin_multi)");             \
        CHECK(h, (j) >= 0 && (j) < 2 * (h)->groups, (h)->groups == 2 ? name ": right-hand side %d out of range (0 .. 3)"  \
                                                                    : name ": right-hand side %d out of range (0, 1)", (int)(j)); \
    } while (0)

// ---- each column of a pipelined two-RHS session stopped at its own threshold ----
int prcg_set_stop_rhs(prcg_t* h, int nrhs, const double* rr_stop) {
    if (!h) return PRCG_EINVAL;
    if (!rr_stop) { h->stop_req[kStopRhs] = Handle::StopRequest{}; return PRCG_OK; }
    CHECK(h, nrhs == 2, "prcg_set_stop_rhs: nrhs = %d: only the pipelined two-RHS session (prcg_solve_begin_multi_pipe) can stop its columns: "
                        "exactly 2 thresholds (NULL clears them)", nrhs);
    for (int c = 0; c < 2; ++c)
        CHECK(h, std::isfinite(rr_stop[c]) && rr_stop[c] >= 0.0, "prcg_set_stop_rhs: rr_stop[%d] = %g: the threshold of column %d must be finite "
              "and >= 0 (a bound on r.r; 0 stops on an exactly zero residual or on breakdown only)", c, rr_stop[c], c);
    h->stop_req[kStopRhs].set = true; h->stop_req[kStopRhs].thr[0] = rr_stop[0]; h->stop_req[kStopRhs].thr[1] = rr_stop[1];
    return PRCG_OK;
}

int prcg_get_stops_rhs(prcg_t* h, int32_t* k_stop, int32_t* status) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, h->in_session && h->rhs2, "prcg_get_stops_rhs: no open multi-RHS session (prcg_solve_begin_multi_pipe)");
    CHECK(h, k_stop && status, "prcg_get_stops_rhs: null buffer");
    int rc = prcg_sync(h);
    if (rc) return rc;
    for (int c = 0; c < 2 * h->groups; ++c) {
        const bool stopped = h->column_stopped(c);
        k_stop[c] = stopped ? h->stopped_k[c] : -1;
        status[c] = stopped ? h->stop_status[c] : 0;
    }
    return PRCG_OK;
}

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
    const PairBufs& G = h->grp[j / 2];
    const DevBuf* src = which == PRCG_VEC_X ? &G.x : which == PRCG_VEC_R ? &G.r : which == PRCG_VEC_P ? &G.p :
                        which == PRCG_VEC_S ? &G.s : (which == PRCG_VEC_RT && h->prec) ? &G.rt :
                        (which == PRCG_VEC_ST && h->prec && pr2(h)) ? &G.st : nullptr;
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
    const int first = row0(h, j / 2);
    if (h->column_stopped(j) && k > h->stopped_k[j]) {      // beyond the column's stop: not part of its run
        for (int q = 0; q < kNS; ++q) out[q] = 0.0;
        return PRCG_OK;
    }
    j %= 2;
    if ((rc = d2h(h, row, dots_at(h, first + (two_rows(h) ? 2 * k + j : k)), kNS))) return rc;
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
    const int first = row0(h, j / 2);
    if (h->column_stopped(j) && k > h->stopped_k[j]) { out[0] = out[1] = out[2] = 0.0; return PRCG_OK; }   // (as the scalars)
    j %= 2;
    if ((rc = d2h(h, row, coef_at(h, first + (two_rows(h) ? 2 * k + j : k)), kCoefStride))) return rc;
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
    if ((rc = d2h(h, all.data(), dots_at(h, row0(h, j / 2)), (int64_t)(m + 1) * rows * kNS))) return rc;
    // (a column stopped at its threshold: its history ends with the entry of its stop)
    const int last = (h->column_stopped(j) && h->stopped_k[j] < h->k) ? h->stopped_k[j] : h->k;
    j %= 2;
    for (int k = 0; k < m; ++k) {
        const double rr = two_rows(h) ? all[(size_t)(2 * k + j) * kNS + PRCG_S_RR] : all[(size_t)k * kNS + kHs2Rr + 2 * j];
        hist[k] = k <= last ? std::sqrt(rr) : 0.0;
    }
    return PRCG_OK;
}

}  // extern "C"
