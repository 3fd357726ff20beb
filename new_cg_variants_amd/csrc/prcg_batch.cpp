// A batch of small independent systems A_s x_s = b_s, every one solved by the one-workgroup solver (k_small_pipe_pr_batch /
// k_small_hs_batch, prcg_small.hip), all of them in the same launch: blockIdx.x selects the system.  Implements the prcg_batch_*
// entries of include/prcg.h and the planner hook prcg_plan_small_batch of include/prcg_test.h.  Host code only.
//
// Layout on the device: the matrices concatenated (every matrix uploaded once, however many systems use it); per session the
// systems' state concatenated in system order -- pipelined: the pairs (x,p) and (r,s); Hestenes-Stiefel: x, r, p, s; a session
// begun with prcg_batch_begin_jacobi adds the pairs (r~,s~) (pipelined) and the systems' inverse diagonals d; one begun with
// prcg_batch_begin_block_jacobi the same pairs, the packed inverses of every system's blocks and one table entry per row
// (SmallBlocks::tab, derived here from the partitions in O(n)) --, one
// scalar history [max_iter+1][PRCG_NUM_SCALARS] and one coefficient history [max_iter+1][4] per system, and one descriptor
// (SmallArgs) per system, sorted by LAUNCH GROUP: the systems whose matrix lives in registers (mode 1) first, then those
// whose matrix lives in LDS (mode 0); inside a group in system order.  An iteration call is one launch per group on the
// handle's compute stream, begin one initialisation launch per group.  Nothing a system computes depends on its group's other
// members: the launch's dynamic LDS is the group's largest need, each workgroup carves it by its own n and nnz.
//
// Thresholds set with prcg_batch_set_stop are kept on the host; a session begun while they are set adds one SmallStop per system
// (sorted like the descriptors) and one stop word {iteration, status} per system (in SYSTEM order), and its iteration calls hand
// them to the launch (SmallBatchArgs::stop), which then applies the stopping rule (prcg_kernels.h: SmallStop) inside each
// workgroup.  A session begun without them launches the kernels without the rule.
#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdint>
#include <new>
#include <vector>

#include "../../include/prcg.h"
#include "../../include/prcg_test.h"
#include "prcg_handle.h"

using namespace prcg;

namespace {

struct Buf {
    void* p = nullptr;
    size_t cap = 0;
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    ~Buf() { if (p) (void)hipFree(p); }
    hipError_t ensure(size_t bytes) {      // (contents undefined)
        if (bytes == 0) bytes = 16;
        if (p && cap >= bytes) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) { p = nullptr; return e; }
        cap = bytes;
        return hipSuccess;
    }
    double* d() const { return static_cast<double*>(p); }
};

// launch groups of a batch: mode 1 first, then mode 0; group ids count the groups that exist.  prec: the fit rule of the
// preconditioned bodies (kSmallPrecJacobi and kSmallPrecBlocks: 128 B more LDS)
int plan_groups(int n_sys, const int64_t* n, const int64_t* nnz, const int32_t* max_row_len, int32_t* mode_out, int32_t* group_out,
                int prec = kSmallPrecNone) {
    bool have[2] = {false, false};
    for (int s = 0; s < n_sys; ++s) {
        int mode = 0;
        if (nnz[s] < 0 || !small_fits(n[s], nnz[s], max_row_len[s], &mode, prec)) return -s - 1;
        mode_out[s] = mode;
        have[mode] = true;
    }
    for (int s = 0; s < n_sys; ++s) group_out[s] = mode_out[s] == 1 ? 0 : (have[1] ? 1 : 0);
    return (have[0] ? 1 : 0) + (have[1] ? 1 : 0);
}

}  // namespace

struct prcg_batch {
    prcg_t* h = nullptr;
    int dev = 0;
    hipStream_t sc = nullptr;
    int n_sys = 0;
    std::vector<int> n, nnz, mode, slot, mrl;      // per system: rows, nonzeros, mode, position of its descriptor, longest row
    std::vector<int64_t> voff;                     // per system (+1): first row in the concatenated vectors
    std::vector<const int*> indptr, col;           // per system: its matrix on the device
    std::vector<const double*> val;
    int count[2] = {0, 0};                         // systems of mode 0 / mode 1
    size_t lds[2][3] = {};                         // [mode][prec]: largest small_lds_bytes of the mode's members
    Buf m_indptr, m_col, m_val;                    // the matrices, concatenated
    Buf state, rhs, x0, dinv, dots, coef, desc, init, jac, tmp, stop, words;
    Buf binv, btab, blk;                           // block Jacobi: the packed inverses, the per-row table, one SmallBlocks per system
    std::vector<double> rr_stop;                   // per system: the threshold on r.r of sessions begun from now on (empty: none)
    // ---- session ----
    bool in_session = false, hs = false, jacobi = false, stopping = false;      // jacobi: preconditioned, by d or by blocks
    int prec = kSmallPrecNone;
    int variant = 0, max_iter = 0, k = 0;
    uint32_t hist_mask = 0;

    int64_t N() const { return voff[(size_t)n_sys]; }
    double* dots_of(int s) const { return dots.d() + (size_t)s * (max_iter + 1) * kNS; }
    double* coef_of(int s) const { return coef.d() + (size_t)s * (max_iter + 1) * kCoefStride; }
    // first descriptor of a mode's launch: mode 1 leads
    const SmallArgs* desc_of(int m) const { return static_cast<const SmallArgs*>(desc.p) + (m == 1 ? 0 : count[1]); }
    const SmallInit* init_of(int m) const { return static_cast<const SmallInit*>(init.p) + (m == 1 ? 0 : count[1]); }
    const SmallJacobi* jac_of(int m) const { return static_cast<const SmallJacobi*>(jac.p) + (m == 1 ? 0 : count[1]); }
    const SmallBlocks* blk_of(int m) const { return static_cast<const SmallBlocks*>(blk.p) + (m == 1 ? 0 : count[1]); }
    const SmallStop* stop_of(int m) const { return static_cast<const SmallStop*>(stop.p) + (m == 1 ? 0 : count[1]); }
};

extern "C" {

int prcg_plan_small_batch(int n_sys, const int64_t* n, const int64_t* nnz, const int32_t* max_row_len, int32_t* mode_out,
                          int32_t* group_out) {
    if (n_sys < 1 || !n || !nnz || !max_row_len || !mode_out || !group_out) return 0;
    return plan_groups(n_sys, n, nnz, max_row_len, mode_out, group_out);
}

int prcg_plan_small_batch_jacobi(int n_sys, const int64_t* n, const int64_t* nnz, const int32_t* max_row_len, int32_t* mode_out,
                                 int32_t* group_out) {
    if (n_sys < 1 || !n || !nnz || !max_row_len || !mode_out || !group_out) return 0;
    return plan_groups(n_sys, n, nnz, max_row_len, mode_out, group_out, kSmallPrecJacobi);
}

int prcg_plan_small_batch_blocks(int n_sys, const int64_t* n, const int64_t* nnz, const int32_t* max_row_len, int32_t* mode_out,
                                 int32_t* group_out) {
    if (n_sys < 1 || !n || !nnz || !max_row_len || !mode_out || !group_out) return 0;
    return plan_groups(n_sys, n, nnz, max_row_len, mode_out, group_out, kSmallPrecBlocks);
}

int prcg_batch_create(prcg_t* h, int n_mat, const int64_t* rows_off, const int64_t* nnz_off, const int32_t* indptr,
                      const int32_t* indices, const double* data, int n_sys, const int32_t* mat_of, prcg_batch_t** out) {
    if (!h) return PRCG_EINVAL;
    CHECK(h, out, "prcg_batch_create: null output pointer");
    *out = nullptr;
    CHECK(h, rows_off && nnz_off && indptr && indices && data && mat_of, "prcg_batch_create: null pointer argument");
    CHECK(h, n_sys >= 1, "prcg_batch_create: n_sys = %d: a batch holds at least one system", n_sys);
    CHECK(h, n_mat >= 1, "prcg_batch_create: n_mat = %d: a batch holds at least one matrix", n_mat);
    CHECK(h, !h->multi(), "prcg_batch_create: the handle carries a communicator: a batch runs on one GPU, on a handle without one");
    CHECK(h, rows_off[0] == 0 && nnz_off[0] == 0, "prcg_batch_create: inconsistent offsets: rows_off[0] and nnz_off[0] must be 0");
    std::vector<int> mrl((size_t)n_mat, 0);
    for (int m = 0; m < n_mat; ++m) {
        const int64_t nm = rows_off[m + 1] - rows_off[m], zm = nnz_off[m + 1] - nnz_off[m];
        CHECK(h, nm >= 1 && zm >= 0 && nm < (1 << 30) && zm < (1ll << 31),
               "prcg_batch_create: inconsistent offsets: matrix %d has %lld rows and %lld nonzeros", m, (long long)nm, (long long)zm);
        const int32_t* ip = indptr + rows_off[m] + m;            // n_m + 1 entries per matrix
        CHECK(h, ip[0] == 0 && ip[nm] == zm, "prcg_batch_create: inconsistent offsets: indptr of matrix %d runs from %d to %d, its "
               "nonzeros number %lld (indptr is zero-based per matrix)", m, ip[0], ip[nm], (long long)zm);
        for (int64_t i = 0; i < nm; ++i) {
            CHECK(h, ip[i + 1] >= ip[i], "prcg_batch_create: inconsistent offsets: indptr of matrix %d decreases at row %lld", m, (long long)i);
            if (ip[i + 1] - ip[i] > mrl[(size_t)m]) mrl[(size_t)m] = ip[i + 1] - ip[i];
        }
        const int32_t* ci = indices + nnz_off[m];
        for (int64_t q = 0; q < zm; ++q)
            CHECK(h, ci[q] >= 0 && ci[q] < nm, "prcg_batch_create: column index %d of matrix %d (nonzero %lld) lies outside its %lld columns",
                   ci[q], m, (long long)q, (long long)nm);
    }
    std::vector<int64_t> sn((size_t)n_sys), sz((size_t)n_sys);
    std::vector<int32_t> sl((size_t)n_sys), mode((size_t)n_sys), group((size_t)n_sys);
    for (int s = 0; s < n_sys; ++s) {
        const int m = mat_of[s];
        CHECK(h, m >= 0 && m < n_mat, "prcg_batch_create: mat_of[%d] = %d lies outside [0, %d): system %d names no matrix", s, m, n_mat, s);
        sn[(size_t)s] = rows_off[m + 1] - rows_off[m]; sz[(size_t)s] = nnz_off[m + 1] - nnz_off[m]; sl[(size_t)s] = mrl[(size_t)m];
    }
    const int ng = plan_groups(n_sys, sn.data(), sz.data(), sl.data(), mode.data(), group.data());
    if (ng < 0) {
        const int s = -ng - 1;
        return fail(h, PRCG_EINVAL, "prcg_batch_create: system %d (n = %lld, nnz = %lld, longest row %d) does not fit the one-workgroup "
                          "solver (at most 4096 rows, and the matrix in registers or in LDS beside the vectors); a batch has no other "
                          "schedule: solve it in a session of its own", s, (long long)sn[(size_t)s], (long long)sz[(size_t)s], sl[(size_t)s]);
    }
    prcg_batch* b = new (std::nothrow) prcg_batch();
    if (!b) return fail(h, PRCG_ENOMEM, "out of host memory");
    struct Guard { prcg_batch* b; ~Guard() { delete b; } } guard{b};      // (released on success)
    b->h = h; b->dev = h->dev; b->sc = h->sc; b->n_sys = n_sys;
    HIPCHK(h, hipSetDevice(b->dev));
    const int64_t rows_all = rows_off[n_mat], nnz_all = nnz_off[n_mat];
    HIPCHK(h, b->m_indptr.ensure((size_t)(rows_all + n_mat) * sizeof(int32_t)));
    HIPCHK(h, b->m_col.ensure((size_t)nnz_all * sizeof(int32_t)));
    HIPCHK(h, b->m_val.ensure((size_t)nnz_all * sizeof(double)));
    HIPCHK(h, hipMemcpyAsync(b->m_indptr.p, indptr, (size_t)(rows_all + n_mat) * sizeof(int32_t), hipMemcpyHostToDevice, b->sc));
    if (nnz_all) {
        HIPCHK(h, hipMemcpyAsync(b->m_col.p, indices, (size_t)nnz_all * sizeof(int32_t), hipMemcpyHostToDevice, b->sc));
        HIPCHK(h, hipMemcpyAsync(b->m_val.p, data, (size_t)nnz_all * sizeof(double), hipMemcpyHostToDevice, b->sc));
    }
    HIPCHK(h, hipStreamSynchronize(b->sc));
    b->n.resize((size_t)n_sys); b->nnz.resize((size_t)n_sys); b->mode.resize((size_t)n_sys); b->slot.resize((size_t)n_sys);
    b->mrl.resize((size_t)n_sys);
    b->voff.assign((size_t)n_sys + 1, 0);
    b->indptr.resize((size_t)n_sys); b->col.resize((size_t)n_sys); b->val.resize((size_t)n_sys);
    for (int s = 0; s < n_sys; ++s) {
        const int m = mat_of[s], md = mode[(size_t)s];
        b->n[(size_t)s] = (int)sn[(size_t)s]; b->nnz[(size_t)s] = (int)sz[(size_t)s]; b->mode[(size_t)s] = md;
        b->mrl[(size_t)s] = sl[(size_t)s];
        b->voff[(size_t)s + 1] = b->voff[(size_t)s] + sn[(size_t)s];
        b->indptr[(size_t)s] = static_cast<const int*>(b->m_indptr.p) + rows_off[m] + m;
        b->col[(size_t)s] = static_cast<const int*>(b->m_col.p) + nnz_off[m];
        b->val[(size_t)s] = b->m_val.d() + nnz_off[m];
        ++b->count[md];
        for (int j = 0; j < 3; ++j) {
            const size_t need = small_lds_bytes(b->n[(size_t)s], b->nnz[(size_t)s], md, j);
            if (need > b->lds[md][j]) b->lds[md][j] = need;
        }
    }
    int at[2] = {b->count[1], 0};                  // descriptors: mode 1 first, then mode 0, each in system order
    for (int s = 0; s < n_sys; ++s) b->slot[(size_t)s] = at[b->mode[(size_t)s]]++;
    guard.b = nullptr;
    *out = b;
    return PRCG_OK;
}

void prcg_batch_destroy(prcg_batch_t* b) {
    if (!b) return;
    (void)hipSetDevice(b->dev);
    (void)hipStreamSynchronize(b->sc);
    delete b;
}

}  // extern "C"

// the blocks of prcg_batch_begin_block_jacobi as the caller passes them
struct BlockArgs { const int64_t* nblk_off; const int64_t* block_ptr; const double* inv_blocks; };

// prcg_batch_begin, prcg_batch_begin_jacobi (prec = kSmallPrecJacobi: inv_diag is an argument) and prcg_batch_begin_block_jacobi
// (prec = kSmallPrecBlocks: blocks is); fn names the entry in the error texts
static int batch_begin(prcg_batch_t* b, const char* fn, int prec, int variant, const double* rhs, const double* x0, const double* inv_diag,
                       const BlockArgs* blocks, int max_iter, uint32_t hist_mask) {
    if (!b) return PRCG_EINVAL;
    prcg_t* h = b->h;
    const bool jacobi = prec != kSmallPrecNone, blk = prec == kSmallPrecBlocks;
    CHECK(h, variant == PRCG_PIPE_PR || variant == PRCG_PIPE_PR_M || variant == PRCG_HS,
           "%s: variant %d is not served by a batch (PRCG_PIPE_PR, PRCG_PIPE_PR_M, PRCG_HS: the one-workgroup solver's)", fn, variant);
    if (blk) CHECK(h, rhs && x0 && blocks->nblk_off && blocks->block_ptr && blocks->inv_blocks,
                   "%s: null rhs, x0, nblk_off, block_ptr or inv_blocks", fn);
    else CHECK(h, rhs && x0 && (inv_diag || !jacobi), jacobi ? "%s: null rhs, x0 or inv_diag" : "%s: null rhs or x0", fn);
    CHECK(h, max_iter >= 1, "%s: max_iter = %d, must be at least 1", fn, max_iter);
    CHECK(h, (hist_mask & ~PRCG_HIST_UPDATED_RESIDUAL_2_NORM) == 0,
           "%s: history bits %u: a batch records the updated residual only (PRCG_HIST_UPDATED_RESIDUAL_2_NORM or 0)", fn, hist_mask);
    // block Jacobi: the partitions, and from them one table entry per row and the size of the packed inverses
    std::vector<int2> tab;
    std::vector<int64_t> inv_off;                  // per system (+1): first double of its inverses in inv_blocks
    if (blk) {
        const int64_t* off = blocks->nblk_off;
        CHECK(h, off[0] == 0, "%s: nblk_off[0] is %lld, not 0", fn, (long long)off[0]);
        for (int s = 0; s < b->n_sys; ++s)
            CHECK(h, off[s + 1] >= off[s], "%s: nblk_off decreases at system %d (%lld after %lld)", fn, s, (long long)off[s + 1], (long long)off[s]);
        for (int s = 0; s < b->n_sys; ++s) {
            const int64_t nb = off[s + 1] - off[s], n = b->n[(size_t)s];
            const int64_t* ptr = blocks->block_ptr + off[s] + s;       // nb + 1 entries per system
            CHECK(h, ptr[0] == 0, "%s: the partition of system %d starts at %lld, not 0 (block_ptr is zero-based per system)", fn, s,
                   (long long)ptr[0]);
            CHECK(h, ptr[nb] == n, "%s: the partition of system %d ends at %lld, not at its n = %lld", fn, s, (long long)ptr[nb], (long long)n);
            for (int64_t k = 0; k < nb; ++k)
                CHECK(h, ptr[k + 1] - ptr[k] >= 1 && ptr[k + 1] - ptr[k] <= 8, "%s: system %d, block %lld has size %lld, outside 1..8", fn, s,
                       (long long)k, (long long)(ptr[k + 1] - ptr[k]));
        }
        for (int s = 0; s < b->n_sys; ++s) {
            int mode = 0;
            CHECK(h, small_fits(b->n[(size_t)s], b->nnz[(size_t)s], b->mrl[(size_t)s], &mode, kSmallPrecBlocks),
                   "%s: system %d (n = %d, nnz = %d) fits the one-workgroup solver without a preconditioner but not with one: "
                   "the preconditioned solver needs %zu bytes of LDS, 128 more, and the cap is 159744", fn, s, b->n[(size_t)s], b->nnz[(size_t)s], small_lds_bytes(b->n[(size_t)s], b->nnz[(size_t)s], 0, kSmallPrecBlocks));
        }
        tab.resize((size_t)b->N());
        inv_off.assign((size_t)b->n_sys + 1, 0);
        for (int s = 0; s < b->n_sys; ++s) {
            const int64_t nb = off[s + 1] - off[s];
            const int64_t* ptr = blocks->block_ptr + off[s] + s;
            int2* row = tab.data() + b->voff[(size_t)s];
            int at = 0;                                // < 8 n <= 32768: offsets inside a system fit an int
            for (int64_t k = 0; k < nb; ++k) {
                const int start = (int)ptr[k], m = (int)(ptr[k + 1] - ptr[k]);
                for (int a = 0; a < m; ++a) row[start + a] = make_int2(start | (m << 16), at + a * m);
                at += m * m;
            }
            inv_off[(size_t)s + 1] = inv_off[(size_t)s] + at;
        }
    }
    for (int s = 0; prec == kSmallPrecJacobi && s < b->n_sys; ++s) {
        int mode = 0;
        CHECK(h, small_fits(b->n[(size_t)s], b->nnz[(size_t)s], b->mrl[(size_t)s], &mode, kSmallPrecJacobi),
               "%s: system %d (n = %d, nnz = %d) fits the one-workgroup solver without a preconditioner but not with one: "
               "the preconditioned solver needs %zu bytes of LDS, 128 more, and the cap is 159744", fn, s, b->n[(size_t)s], b->nnz[(size_t)s],
               small_lds_bytes(b->n[(size_t)s], b->nnz[(size_t)s], 0, kSmallPrecJacobi));
    }
    HIPCHK(h, hipSetDevice(b->dev));
    b->in_session = false;
    const int n_sys = b->n_sys;
    const int64_t N = b->N();
    const size_t D = sizeof(double);
    const bool hs = variant == PRCG_HS;
    HIPCHK(h, b->state.ensure((size_t)(jacobi && !hs ? 6 : 4) * N * D));
    if (blk) {
        HIPCHK(h, b->binv.ensure((size_t)inv_off[(size_t)n_sys] * D));
        HIPCHK(h, b->btab.ensure((size_t)N * sizeof(int2)));
        HIPCHK(h, b->blk.ensure((size_t)n_sys * sizeof(SmallBlocks)));
    } else if (jacobi) {
        HIPCHK(h, b->dinv.ensure((size_t)N * D));
        HIPCHK(h, b->jac.ensure((size_t)n_sys * sizeof(SmallJacobi)));
    }
    HIPCHK(h, b->rhs.ensure((size_t)N * D));
    HIPCHK(h, b->x0.ensure((size_t)N * D));
    HIPCHK(h, b->tmp.ensure((size_t)N * D));
    HIPCHK(h, b->dots.ensure((size_t)n_sys * (max_iter + 1) * kNS * D));
    HIPCHK(h, b->coef.ensure((size_t)n_sys * (max_iter + 1) * kCoefStride * D));
    HIPCHK(h, b->desc.ensure((size_t)n_sys * sizeof(SmallArgs)));
    HIPCHK(h, b->init.ensure((size_t)n_sys * sizeof(SmallInit)));
    const bool stopping = !b->rr_stop.empty();
    if (stopping) {
        HIPCHK(h, b->stop.ensure((size_t)n_sys * sizeof(SmallStop)));
        HIPCHK(h, b->words.ensure((size_t)n_sys * 2 * sizeof(int32_t)));
    }
    b->stopping = stopping;
    b->variant = variant; b->hs = hs; b->jacobi = jacobi; b->prec = prec; b->max_iter = max_iter; b->hist_mask = hist_mask; b->k = 0;
    std::vector<SmallArgs> desc((size_t)n_sys);
    std::vector<SmallInit> init((size_t)n_sys);
    std::vector<SmallJacobi> jac(prec == kSmallPrecJacobi ? (size_t)n_sys : 0);
    std::vector<SmallBlocks> sblk(blk ? (size_t)n_sys : 0);
    std::vector<SmallStop> stop(stopping ? (size_t)n_sys : 0);
    std::vector<int32_t> words(stopping ? (size_t)n_sys * 2 : 0);
    double* st = b->state.d();
    for (int s = 0; s < n_sys; ++s) {
        const int64_t v = b->voff[(size_t)s];
        SmallArgs a{};
        a.n = b->n[(size_t)s]; a.nnz = b->nnz[(size_t)s];
        a.indptr = b->indptr[(size_t)s]; a.col = b->col[(size_t)s]; a.val = b->val[(size_t)s];
        if (hs) { a.xp = st + v; a.rs = st + N + v; a.hs_p = st + 2 * N + v; a.hs_s = st + 3 * N + v; }
        else { a.xp = st + 2 * v; a.rs = st + 2 * N + 2 * v; }
        a.dots = b->dots_of(s); a.coef = b->coef_of(s);
        desc[(size_t)b->slot[(size_t)s]] = a;
        init[(size_t)b->slot[(size_t)s]] = SmallInit{b->rhs.d() + v, b->x0.d() + v};
        // the pairs (r~,s~) follow (x,p) and (r,s); Hestenes-Stiefel holds no r~
        if (blk) sblk[(size_t)b->slot[(size_t)s]] = SmallBlocks{hs ? nullptr : st + 4 * N + 2 * v, static_cast<const int2*>(b->btab.p) + v,
                                                                 b->binv.d() + inv_off[(size_t)s]};
        else if (jacobi) jac[(size_t)b->slot[(size_t)s]] = SmallJacobi{hs ? nullptr : st + 4 * N + 2 * v, b->dinv.d() + v};
        if (stopping) {                                // every system starts as {-1, 0}: running
            stop[(size_t)b->slot[(size_t)s]] = SmallStop{b->rr_stop[(size_t)s], static_cast<int*>(b->words.p) + 2 * s};
            words[(size_t)2 * s] = -1; words[(size_t)2 * s + 1] = 0;
        }
    }
    hipStream_t sc = b->sc;
    HIPCHK(h, hipMemsetAsync(b->dots.p, 0, (size_t)n_sys * (max_iter + 1) * kNS * D, sc));
    HIPCHK(h, hipMemsetAsync(b->coef.p, 0, (size_t)n_sys * (max_iter + 1) * kCoefStride * D, sc));
    HIPCHK(h, hipMemcpyAsync(b->rhs.p, rhs, (size_t)N * D, hipMemcpyHostToDevice, sc));
    HIPCHK(h, hipMemcpyAsync(b->x0.p, x0, (size_t)N * D, hipMemcpyHostToDevice, sc));
    HIPCHK(h, hipMemcpyAsync(b->desc.p, desc.data(), (size_t)n_sys * sizeof(SmallArgs), hipMemcpyHostToDevice, sc));
    HIPCHK(h, hipMemcpyAsync(b->init.p, init.data(), (size_t)n_sys * sizeof(SmallInit), hipMemcpyHostToDevice, sc));
    if (blk) {
        if (inv_off[(size_t)n_sys])
            HIPCHK(h, hipMemcpyAsync(b->binv.p, blocks->inv_blocks, (size_t)inv_off[(size_t)n_sys] * D, hipMemcpyHostToDevice, sc));
        HIPCHK(h, hipMemcpyAsync(b->btab.p, tab.data(), (size_t)N * sizeof(int2), hipMemcpyHostToDevice, sc));
        HIPCHK(h, hipMemcpyAsync(b->blk.p, sblk.data(), (size_t)n_sys * sizeof(SmallBlocks), hipMemcpyHostToDevice, sc));
    } else if (jacobi) {
        HIPCHK(h, hipMemcpyAsync(b->dinv.p, inv_diag, (size_t)N * D, hipMemcpyHostToDevice, sc));
        HIPCHK(h, hipMemcpyAsync(b->jac.p, jac.data(), (size_t)n_sys * sizeof(SmallJacobi), hipMemcpyHostToDevice, sc));
    }
    if (stopping) {
        HIPCHK(h, hipMemcpyAsync(b->stop.p, stop.data(), (size_t)n_sys * sizeof(SmallStop), hipMemcpyHostToDevice, sc));
        HIPCHK(h, hipMemcpyAsync(b->words.p, words.data(), (size_t)n_sys * 2 * sizeof(int32_t), hipMemcpyHostToDevice, sc));
    }
    HIPCHK(h, hipStreamSynchronize(sc));             // (desc / init leave scope; the caller's buffers are theirs again)
    for (int m = 1; m >= 0; --m) {                 // one initialisation launch per group
        if (!b->count[m]) continue;
        if (launch_small_batch_init(sc, b->desc_of(m), b->init_of(m), prec == kSmallPrecJacobi ? b->jac_of(m) : nullptr, b->count[m], hs,
                                    blk ? b->blk_of(m) : nullptr) < 0)
            return fail(h, PRCG_EHIP, "%s: kernel launch failed", fn);
    }
    HIPCHK(h, hipStreamSynchronize(sc));
    b->in_session = true;
    return PRCG_OK;
}

extern "C" {

int prcg_batch_begin(prcg_batch_t* b, int variant, const double* rhs, const double* x0, int max_iter, uint32_t hist_mask) {
    return batch_begin(b, "prcg_batch_begin", kSmallPrecNone, variant, rhs, x0, nullptr, nullptr, max_iter, hist_mask);
}

int prcg_batch_begin_jacobi(prcg_batch_t* b, int variant, const double* rhs, const double* x0, const double* inv_diag, int max_iter,
                            uint32_t hist_mask) {
    return batch_begin(b, "prcg_batch_begin_jacobi", kSmallPrecJacobi, variant, rhs, x0, inv_diag, nullptr, max_iter, hist_mask);
}

int prcg_batch_begin_block_jacobi(prcg_batch_t* b, int variant, const double* rhs, const double* x0, const int64_t* nblk_off,
                                  const int64_t* block_ptr, const double* inv_blocks, int max_iter, uint32_t hist_mask) {
    const BlockArgs blocks{nblk_off, block_ptr, inv_blocks};
    return batch_begin(b, "prcg_batch_begin_block_jacobi", kSmallPrecBlocks, variant, rhs, x0, nullptr, &blocks, max_iter, hist_mask);
}

int prcg_batch_iterate(prcg_batch_t* b, int iters) {
    if (!b) return PRCG_EINVAL;
    prcg_t* h = b->h;
    CHECK(h, b->in_session, "prcg_batch_iterate: no open session");
    CHECK(h, iters >= 0, "prcg_batch_iterate: negative count");
    CHECK(h, b->k + iters <= b->max_iter, "prcg_batch_iterate: %d more iterations exceed max_iter=%d (k=%d)", iters, b->max_iter, b->k);
    if (iters == 0) return PRCG_OK;
    HIPCHK(h, hipSetDevice(b->dev));
    const int meurant = b->variant == PRCG_PIPE_PR_M ? 1 : 0;
    for (int m = 1; m >= 0; --m) {                 // one launch per group: every system advances by iters
        if (!b->count[m]) continue;
        const SmallBatchArgs g{b->desc_of(m), b->prec == kSmallPrecJacobi ? b->jac_of(m) : nullptr, b->stopping ? b->stop_of(m) : nullptr, b->k,
                               iters, meurant};
        const int rc = launch_small_batch(b->sc, g, b->count[m], m, b->lds[m][b->prec], b->hs, b->prec == kSmallPrecBlocks ? b->blk_of(m) : nullptr);
        if (rc < 0) return fail(h, PRCG_EHIP, "prcg_batch_iterate: kernel launch failed (or the dynamic-LDS attribute could not be set)");
    }
    b->k += iters;
    return PRCG_OK;
}

int prcg_batch_sync(prcg_batch_t* b) {
    if (!b) return PRCG_EINVAL;
    HIPCHK(b->h, hipSetDevice(b->dev));
    HIPCHK(b->h, hipStreamSynchronize(b->sc));
    return PRCG_OK;
}

int prcg_batch_iteration(const prcg_batch_t* b) { return b ? b->k : -1; }

int prcg_batch_set_stop(prcg_batch_t* b, const double* rr_stop) {
    if (!b) return PRCG_EINVAL;
    prcg_t* h = b->h;
    if (!rr_stop) { b->rr_stop.clear(); return PRCG_OK; }
    for (int s = 0; s < b->n_sys; ++s)
        CHECK(h, std::isfinite(rr_stop[s]) && rr_stop[s] >= 0.0, "prcg_batch_set_stop: rr_stop[%d] = %g: the threshold of system %d must be "
               "finite and >= 0 (a bound on r.r; 0 stops on an exactly zero residual only)", s, rr_stop[s], s);
    b->rr_stop.assign(rr_stop, rr_stop + b->n_sys);
    return PRCG_OK;
}

int prcg_batch_get_stops(prcg_batch_t* b, int32_t* k_stop, int32_t* status) {
    if (!b) return PRCG_EINVAL;
    prcg_t* h = b->h;
    CHECK(h, b->in_session, "prcg_batch_get_stops: no open session");
    CHECK(h, k_stop && status, "prcg_batch_get_stops: null buffer");
    HIPCHK(h, hipSetDevice(b->dev));
    HIPCHK(h, hipStreamSynchronize(b->sc));
    if (!b->stopping) {
        for (int s = 0; s < b->n_sys; ++s) { k_stop[s] = -1; status[s] = 0; }
        return PRCG_OK;
    }
    std::vector<int32_t> words((size_t)b->n_sys * 2);
    HIPCHK(h, hipMemcpyAsync(words.data(), b->words.p, words.size() * sizeof(int32_t), hipMemcpyDeviceToHost, b->sc));
    HIPCHK(h, hipStreamSynchronize(b->sc));
    for (int s = 0; s < b->n_sys; ++s) { k_stop[s] = words[(size_t)2 * s]; status[s] = words[(size_t)2 * s + 1]; }
    return PRCG_OK;
}

static int batch_d2h(prcg_batch_t* b, double* dst, const double* src, int64_t count) {
    HIPCHK(b->h, hipMemcpyAsync(dst, src, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, b->sc));
    HIPCHK(b->h, hipStreamSynchronize(b->sc));
    return PRCG_OK;
}

int prcg_batch_get_vector(prcg_batch_t* b, int which, int s, double* out) {
    if (!b) return PRCG_EINVAL;
    prcg_t* h = b->h;
    CHECK(h, b->in_session && out, "prcg_batch_get_vector: no session or null buffer");
    CHECK(h, s >= 0 && s < b->n_sys, "prcg_batch_get_vector: system %d outside [0, %d)", s, b->n_sys);
    const bool tilde = which == PRCG_VEC_RT || which == PRCG_VEC_ST;
    CHECK(h, !tilde || (b->jacobi && !b->hs), "prcg_batch_get_vector: vector %d (PRCG_VEC_RT / _ST) is held by a pipelined session begun "
           "with prcg_batch_begin_jacobi or prcg_batch_begin_block_jacobi only: this session is %s", which, b->jacobi ? "Hestenes-Stiefel, which forms r~ anew in every iteration"
                                                                                     : "unpreconditioned");
    CHECK(h, tilde || which == PRCG_VEC_X || which == PRCG_VEC_R || which == PRCG_VEC_P || which == PRCG_VEC_S,
           "prcg_batch_get_vector: vector %d is not part of a batch session (PRCG_VEC_X, _R, _P, _S)", which);
    HIPCHK(h, hipSetDevice(b->dev));
    const int64_t N = b->N(), v = b->voff[(size_t)s], n = b->n[(size_t)s];
    if (tilde) {                                   // the pair array (r~,s~) follows (x,p) and (r,s)
        launch_copy(b->sc, b->tmp.d(), 1, b->state.d() + 4 * N + 2 * v + (which == PRCG_VEC_ST ? 1 : 0), 2, n);
        return batch_d2h(b, out, b->tmp.d(), n);
    }
    const int idx = which == PRCG_VEC_X ? 0 : which == PRCG_VEC_R ? 1 : which == PRCG_VEC_P ? 2 : 3;
    if (b->hs) return batch_d2h(b, out, b->state.d() + idx * N + v, n);
    // pairs (x,p) and (r,s): component (idx >> 1) of pair array (idx & 1)
    launch_copy(b->sc, b->tmp.d(), 1, b->state.d() + (idx & 1) * 2 * N + 2 * v + (idx >> 1), 2, n);
    return batch_d2h(b, out, b->tmp.d(), n);
}

int prcg_batch_get_solutions(prcg_batch_t* b, double* x_cat) {
    if (!b) return PRCG_EINVAL;
    prcg_t* h = b->h;
    CHECK(h, b->in_session && x_cat, "prcg_batch_get_solutions: no session or null buffer");
    HIPCHK(h, hipSetDevice(b->dev));
    const int64_t N = b->N();
    if (b->hs) return batch_d2h(b, x_cat, b->state.d(), N);
    launch_copy(b->sc, b->tmp.d(), 1, b->state.d(), 2, N);       // the x of every (x,p) pair, all systems at once
    return batch_d2h(b, x_cat, b->tmp.d(), N);
}

int prcg_batch_get_scalars(prcg_batch_t* b, int k, int s, double* out) {
    if (!b) return PRCG_EINVAL;
    prcg_t* h = b->h;
    CHECK(h, b->in_session && out && k >= 0 && k <= b->max_iter && s >= 0 && s < b->n_sys, "prcg_batch_get_scalars: bad argument");
    HIPCHK(h, hipSetDevice(b->dev));
    return batch_d2h(b, out, b->dots_of(s) + (size_t)k * kNS, kNS);
}

int prcg_batch_get_coefficients(prcg_batch_t* b, int k, int s, double* out) {
    if (!b) return PRCG_EINVAL;
    prcg_t* h = b->h;
    CHECK(h, b->in_session && out && k >= 1 && k <= b->max_iter && s >= 0 && s < b->n_sys, "prcg_batch_get_coefficients: bad argument");
    HIPCHK(h, hipSetDevice(b->dev));
    return batch_d2h(b, out, b->coef_of(s) + (size_t)k * kCoefStride, 3);
}

int prcg_batch_get_history(prcg_batch_t* b, int s, double* hist) {
    if (!b) return PRCG_EINVAL;
    prcg_t* h = b->h;
    CHECK(h, b->in_session && hist, "prcg_batch_get_history: no session or null buffer");
    CHECK(h, s >= 0 && s < b->n_sys, "prcg_batch_get_history: system %d outside [0, %d)", s, b->n_sys);
    if (!(b->hist_mask & PRCG_HIST_UPDATED_RESIDUAL_2_NORM)) return PRCG_OK;
    HIPCHK(h, hipSetDevice(b->dev));
    const int m = b->max_iter;
    std::vector<double> all((size_t)(m + 1) * kNS);
    if (int rc = batch_d2h(b, all.data(), b->dots_of(s), (int64_t)(m + 1) * kNS)) return rc;
    int last = b->k;                               // a stopped system has entries up to its stop iteration
    if (b->stopping) {
        int32_t word[2];
        HIPCHK(h, hipMemcpyAsync(word, static_cast<const int32_t*>(b->words.p) + 2 * s, sizeof(word), hipMemcpyDeviceToHost, b->sc));
        HIPCHK(h, hipStreamSynchronize(b->sc));
        if (word[0] >= 0 && word[0] < last) last = word[0];
    }
    for (int k = 0; k < m; ++k) hist[k] = k <= last ? std::sqrt(all[(size_t)k * kNS + PRCG_S_RR]) : 0.0;
    return PRCG_OK;
}

}  // extern "C"
