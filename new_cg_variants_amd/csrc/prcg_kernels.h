// Launch wrappers of the gfx950 kernels (definitions: prcg_kernels.hip and, one file per kernel family, prcg_win.hip, prcg_sell.hip,
// prcg_blockjac.hip, prcg_rhs2.hip, prcg_small.hip).
// Internal to libprcg.so -- the public boundary is include/prcg.h.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "prcg_geometry.h"

namespace prcg {

// ---- launch geometry (tile geometry shared with the host planner: prcg_geometry.h) ----
constexpr int kMaxGridBlocks = 2048;                // 8 blocks x 256 CUs
constexpr int kPartialStride = 8;                   // doubles per block in a partials array

// ---- direct peer exchange over xGMI (multi-rank one-launch schedule) ------------------------
// Every rank owns one EXCHANGE BUFFER (fine-grained device memory, mapped into every other rank's process with
// hipIpc): per parity (iteration & 1) one 64-byte SLOT per rank -- that rank's five partial inner products of the
// iteration and a 64-bit counter -- and a GHOST AREA that the neighbours' launches fill with the rows this rank needs.
// Launch k of a rank stores with system scope straight into the consumers' buffers: the rows of iteration k its tiles
// update, as soon as a tile is done.  Its COMMUNICATION WAVE (wave 0 of workgroup 0; takes no tiles) first adds the
// partial sums launch k-1 left (kernel boundary: complete, and launch k-1's row stores have arrived), sends them as
// the rank's slot of iteration k-1 into EVERY rank's buffer, waits until all R slots of its own buffer carry that
// counter, adds them in rank order -- the same bits on every rank -- and publishes the sums to the other waves, which
// meanwhile compute the part of the iteration that needs neither (products of their first tiles).  The tiles that
// read ghost rows come last and read them from the rank's own buffer.  No collective, no communication stream, one
// host call per iteration.
//   layout (doubles):  slot(par, q) at (par * R + q) * 8 : [5 sums, pad, pad, counter]
//                      ghost(par)   at 16 * R + par * 2 * (ghost_cap + 64) : ghost_cap pairs (+ 64 spare: a window page)
//   counter = epoch | (k + 1): epoch = session number << 32 (stale slots of an earlier session are smaller)
constexpr int kMaxPeerRanks = 16;
struct PeerDev {
    double* mine;                       // this rank's exchange buffer
    double* peer[kMaxPeerRanks];        // every rank's exchange buffer as mapped here (peer[rank] == mine)
    const int2* tile_send;              // per tile of the table in use: [first, end) of its entries in send_ent
    const int4* send_ent;               // {local row, destination rank, index in the destination's ghost area, 0}, by tile
    int rank, nranks, n_own, ghost_cap;
    unsigned long long epoch;
    int n_send;                         // entries in send_ent
};
__host__ __device__ inline int peer_slot_off(int nranks, int par, int q) { return (par * nranks + q) * 8; }
__host__ __device__ inline long long peer_ghost_off(int nranks, int ghost_cap, int par) {
    return 16LL * nranks + (long long)par * 2 * (ghost_cap + 64);
}
inline size_t peer_buffer_doubles(int nranks, int ghost_cap) { return (size_t)peer_ghost_off(nranks, ghost_cap, 2); }

// partial inner products of the previous one-launch iteration (see launch_pipe_fused)
// (+ the in-place operands of the Jacobi / 'p' flavours, see FusedState)
struct FusedPrev {
    const double* prev_partials; int nprev; double* dots_prev_out; double* rs; double* w; double* wt;
    // multi-rank one-launch schedule: the inner products of the previous iteration arrive WHILE this launch
    // runs (reduced across ranks on the communication stream, published in `pub`: kPubCopies records of 64
    // bytes, each 5 doubles + a 32-bit iteration counter at byte 48, all stored write-through).  Each wave first computes the products of
    // its first tiles, then waits for pub's counter to reach `want`, then applies the deferred updates.
    const double* pub; unsigned want; unsigned* err;
    unsigned* err_host;  // pinned host word a timed-out wave also sets (prcg_iterate reads it without a synchronisation), or null
    const PeerDev* px;   // non-null: direct peer exchange (above) -- the launch's last workgroup sends this rank's partial sums,
                         // its tiles send the rows the neighbours need, workgroup 0 turns the ranks' slots into `pub`
    int nt_int;       // tiles [nt_int, ntiles) touch ghost columns: they are neither computed nor even requested before
                      // the publication has arrived (the ghost rows travel with it)
    const double* dots_old;   // Hestenes-Stiefel product launch: the scalars of iteration k-1 (nu_k1 for b_k = nu_k / nu_k1)
                              // (one-launch predict-and-recompute: the reduced scalars of k-1 when nprev == 0)
    // one-launch predict-and-recompute iteration (launch_win_pr_one): the three vectors the window is formed from
    // (z = r~ or r, zs = s~ or s, the direction p) are read from the *_old arrays and written to the *_new ones
    // (other tiles still stage the old values); x -- and with Jacobi the plain r, s -- are updated in place
    struct PrOne {
        const double* z_old; const double* zs_old; const double* p_old;
        double* z_new; double* zs_new; double* p_new;
        double* x; double* r; double* s; const double* d;
        double* rt; const double* st;      // Ghysels-Vanroose with Jacobi: r~ (updated in place) and s~ of the row
        // PACKED form of the unpreconditioned iteration (kEpiPROneQ): the four values of a row as two 16-byte pairs, (z, zs) in
        // q_old / q_new and (p, x) in px_old / px_new -- window pages: two 16-byte loads per lane instead of three 8-byte ones
        // (the row's own x rides along), row results: two 16-byte stores, each a contiguous kilobyte per wave, instead of
        // four 8-byte ones; the separate arrays above are not touched
        const double* q_old; double* q_new; const double* px_old; double* px_new;
    } pr;
    // ONE launch per iteration of Chronopoulos-Gear / Ghysels-Vanroose (launch_win_cg_one): the p, s (u) update of the
    // previous iteration is deferred INTO this launch -- see the comment there.  z0, z1, z2: the three old vectors the
    // window is formed from (cg: r, w, s; gv: w, t, u), z?n their new buffers (other tiles still stage the old ones);
    // x, p (and r, s for gv) in place; d: inverse diagonal or null; coef_prev: where a, b of the previous iteration go.
    struct Lag {
        const double* z0; const double* z1; const double* z2;
        double* z0n; double* z1n; double* z2n;
        double* x; double* p; double* r; double* s; const double* d; double* coef_prev;
    } lag;
    // deferred (x,p) store of the single-GPU one-launch iteration (window operators): x and p are row-local, so a launch
    // may leave its (x,p) unwritten and the NEXT launch rebuilds them from the unchanged pair in memory, the row's own
    // entry of the old input pairs (r or r~ of the skipped iteration) and that iteration's a, b -- same operands, same
    // expressions, the same bits.  xphase 0: the launch closes itself; 1 (SKIP): no store to XP; 2 (APPLY): rebuild
    // first, xcoef = the skipped iteration's stored coefficients {a, b} (coef[k-1]: the very doubles that launch used).
    int xphase; const double* xcoef;
    // single session stopped at a residual threshold (prcg_set_stop; single-GPU form of the one-launch iteration only): the
    // session's stop word -- two ints in device memory, the layout and the rule of SmallStop below -- or null: no threshold.
    // word_k: the iteration whose scalars this launch's prologue sums or reads (the launch itself is iteration word_k + 1).
    // A launch that finds the session stopped, or stops it, returns before it has written a coefficient or a row: the state of
    // the stop iteration stays as its own launch wrote it (fused_prologue, prcg_device.hpp).
    int* word; double thr; int word_k;
};
// State of the one-launch pipelined iteration (pipe_pr_cg.py:61-75 unpreconditioned, :169-187 Jacobi):
// the two-vector product of the SpMM input pair array `in_old` with the NEXT vector update applied row
// by row.  in = (r,s) unpreconditioned, (r~,s~) with Jacobi; in_new = the same array of the next
// iteration (other rows still gather the old one).  rs: the plain (r,s) pairs with Jacobi (updated in
// place: only the row itself reads them).  w / wt: the stored w, w~ of the 'p' flavours (in place).
struct FusedState {
    const double* in_old; double* in_new; double* xp;
    double* rs; const double* dinv; double* w; double* wt;
    const double* dots_prev; double* coef_out; double* partials;
    int meurant, recompute_w;
    FusedPrev prev;
    int stream_stores; // 1: the row results go out with streaming (nontemporal) stores: vectors far larger than the caches
    int deferred;     // 1: the launch waits in-kernel for prev.pub (communicator sessions, interior tiles)
    hipEvent_t done;  // non-null: the launch's own completion signal is this event (hipExtLaunchKernel): the
                      // communication stream waits for it, and NO marker packet sits between two launches
                      // on the compute stream (a separate hipEventRecord cost ~15 us of idle queue per iteration)
};

// epilogues fused into the single-vector SpMV
enum SpmvEpilogue {
    kEpiNone = 0,
    kEpiDotXY = 1,   // partial[0] += x_i * y_i                       (HS: mu = p.s; e'Ae)
    kEpiPR = 2,      // st = d*y (or y); partials mu=p.s, dl=r.st, gm=st.s   (pr_pcg)
    kEpiPipeFused = 3,   // two-vector only: the next pipelined vector update, fused row by row
    kEpiCG = 4,      // partials nu = r.x, eta = y.x, rr = r.r                 (cg_cg: x = r~, y = w)
    kEpiPipeFusedP = 5,  // ... 'p' flavours: w is the stored recurrence, only u = A s is used from the product
    kEpiPipeFusedJ = 6,  // ... Jacobi, 'pr' flavours: input (r~,s~); w~ = d w, u~ = d u in registers
    kEpiPipeFusedPJ = 7, // ... Jacobi, 'p' flavours
    kEpiHS = 8,      // window kernels only: the Hestenes-Stiefel product launch (launch_win_hs)
    kEpiPROne = 9,   // window kernels only: one-launch predict-and-recompute iteration (launch_win_pr_one)
    kEpiPROneJ = 10, // ... with Jacobi
    kEpiCGW = 11,    // window kernels only: Chronopoulos-Gear product launch, window formed as r - a s (launch_win_cg_w)
    kEpiCGWJ = 12,   // ... with Jacobi: d (r - a s)
    kEpiGVW = 13,    // window kernels only: Ghysels-Vanroose product launch, window formed as w - a u (launch_win_gv_w)
    kEpiGVWJ = 14,   // ... with Jacobi: d (w - a u)
    kEpiCGOne = 15,  // window kernels only: ONE launch per Chronopoulos-Gear iteration (launch_win_cg_one)
    kEpiCGOneJ = 16, // ... with Jacobi
    kEpiGVOne = 17,  // window kernels only: ONE launch per Ghysels-Vanroose iteration (unpreconditioned)
    kEpiPROneQ = 18, // window kernels only: one-launch predict-and-recompute iteration on the PACKED state, pairs (z, zs) and (p, x) (PrOne::q_old, px_old)
    kEpiNoneStop = 19,   // two- and four-vector products only: the plain epilogue, in a launch that may have nothing to do (ProductStop below)
    kEpiDotXYStop = 20,  // sliced rows and CSR-adaptive tiles, one vector: kEpiDotXY in a launch that may have nothing to do (ProductStop below)
};
constexpr bool epi_plain(int e) { return e == kEpiNone || e == kEpiNoneStop; }     // no inner products: nothing but the product is stored
constexpr bool epi_dot_xy(int e) { return e == kEpiDotXY || e == kEpiDotXYStop; }  // partial[0] += x_i * y_i
constexpr bool epi_product_stop(int e) { return e == kEpiNoneStop || e == kEpiDotXYStop; }     // the head of the launch reads ProductStop's word
// The product launch of iteration k of a pipelined two-RHS session whose columns stop at their own thresholds (prcg_set_stop_rhs;
// kEpiNoneStop: instantiations of their own, so that a session without thresholds launches the kernels it always did).  word: the
// stop word of the launch's column, two ints laid out as SmallStop's (below).  The product of iteration k belongs to the state of
// iteration k, so a column that stops AT k still gets it: the launch returns at once, before anything is loaded or stored, only
// if 0 <= word[0] < k.  The four-vector launch (sliced rows) serves both columns: `word` is then column 0's, column 1's follows
// it (word + 2), and the launch returns only if BOTH stopped before k -- otherwise it runs as it is: a frozen column's sources have
// not changed, so its destination is rewritten with the bits it holds.  The word was complete before the launch began (kernel
// boundary); every wave reads the same value through readfirstlane and leaves on a scalar branch.  Travels in FusedPrev::word /
// word_k, which the plain epilogue does not use otherwise.
// kEpiDotXYStop: the product s = A p with mu = p.s of iteration k of a Hestenes-Stiefel session that stops (prcg_set_stop_hs) on sliced
// rows or CSR-adaptive tiles, by the same head: the product of the stop iteration belongs to its state, so the launch returns only
// if the session stopped BEFORE k; then no partial row is written either (the reduction that would sum them returns as well).
struct ProductStop { int* word; int k; };
// How iteration k of a session stops, as the HOST hands it from the session (Session::stop_at, prcg_handle.h) to a launcher: the
// threshold on r.r, the stop word ({iteration, status}: SmallStop's layout and rule, below) and the iteration.  A null word is "no
// threshold": every launcher that takes a StopAt takes it last, defaulted to none, launches with none the kernels it launches for a
// session without a threshold, and with one the stop kernel of its own (so that a session without a threshold launches what it always
// did).  The kernels receive what they always did: SmallStop{thr, word} where a launch DECIDES, ProductStop{word, k} where it only
// skips, or the bare word.
struct SmallStop;
struct StopAt {
    double thr = 0.0; int* word = nullptr; int k = 0;
    explicit operator bool() const { return word != nullptr; }
    SmallStop decides() const;
    ProductStop skips() const { return ProductStop{word, k}; }
};
// what a plain product launch hands its kernel: an empty FusedPrev, with a stop carrying ProductStop in word / word_k
inline FusedPrev product_prev(const StopAt& stop) { FusedPrev fz{}; fz.word = stop.word; fz.word_k = stop.k; return fz; }
constexpr bool epi_pr_one(int e) { return e == kEpiPROne || e == kEpiPROneJ || e == kEpiPROneQ; }
constexpr bool epi_cg_w(int e) { return e == kEpiCGW || e == kEpiCGWJ; }
constexpr bool epi_gv_w(int e) { return e == kEpiGVW || e == kEpiGVWJ; }
// the launches that form their window from several old vectors and update the row's own vectors (FusedPrev::PrOne)
constexpr bool epi_rowset(int e) { return epi_pr_one(e) || epi_cg_w(e) || epi_gv_w(e); }
constexpr bool epi_lag(int e) { return e == kEpiCGOne || e == kEpiCGOneJ || e == kEpiGVOne; }
constexpr bool epi_fused(int e) { return e == kEpiPipeFused || e == kEpiPipeFusedP || e == kEpiPipeFusedJ || e == kEpiPipeFusedPJ; }
constexpr bool epi_prec(int e) { return e == kEpiPipeFusedJ || e == kEpiPipeFusedPJ; }
constexpr bool epi_recompute(int e) { return e == kEpiPipeFused || e == kEpiPipeFusedJ; }

struct CsrDev {
    const int* indptr;
    const int* col;
    const double* val;
    // Device-internal re-encoding of the column indices, built at prcg_set_csr when every
    // tile's columns span < 65536: col16[q] = col[q] - tile_base[tile of q].  Same indices,
    // 2 bytes instead of 4 on the HBM stream (12 -> 10 bytes per nonzero).  Lossless; the
    // arithmetic is untouched.  Null when not built.
    const unsigned short* col16;
    const unsigned char* col8;  // the same with 1 byte, when every tile spans < 256 columns (narrow bands)
    const int* tile_base;      // per tile, same indexing as the tile table
    // Device-internal re-encoding of the VALUES ("value dictionary", built at prcg_set_csr when
    // every streamed tile holds at most kDictMax distinct bit patterns -- stencils, constant
    // off-diagonals): vidx8[q] = index of val[q] in the tile's dictionary vdict[vd[t].x ..+vd[t].y).
    // 1 byte instead of 8 on the HBM stream; the dictionary entries ARE the original doubles, so
    // every product is bit-identical.  Null when not built.
    const unsigned char* vidx8;
    const double* vdict;
    const int2* vd;            // per tile (same indexing as the tile table): {first entry, count}
};

// y = A x over tiles[0..ntiles).  x has ghost room; y has n_rows entries.
// partials: [grid][kPartialStride] doubles (slots 0..2 used by the epilogues) or null.
// returns the grid size used (needed to reduce the partials), <0 on launch failure.
// (A.tile_base / A.vd are indexed like `tiles`: the caller offsets all three together; the
//  narrow encodings are non-null in A only if every tile of the range qualified)
int launch_spmv(hipStream_t st, const CsrDev& A, const Tile* tiles, int ntiles, int steps,
                const double* x, double* y, SpmvEpilogue epi,
                const double* ep_r, const double* ep_d, double* ep_st,
                double* partials, TileKnobs kn = TileKnobs{}, const StopAt& stop = StopAt{});
// (stop: kEpiDotXY only, -1 for any other epilogue -- y = A x with partial[0] += x_i * y_i of a Hestenes-Stiefel session that stops
//  (ProductStop, kEpiDotXYStop): the same product and the same partial rows, or nothing at all)

// [w u] = A [r s] on interleaved pairs.  write_mask: 1 = first, 2 = second, 3 = both.
int launch_spmm2(hipStream_t st, const CsrDev& A, const Tile* tiles, int ntiles, int steps,
                 const double* rs, double* wu, int write_mask, TileKnobs kn = TileKnobs{}, const StopAt& stop = StopAt{});
// (stop: the product of a session that stops (ProductStop, kEpiNoneStop): the same product, or nothing at all)

// One launch per iteration of pipe_pr_cg / pipe_pr_m_cg on ONE GPU: [w u] = A [r s] with the
// vector update of the following iteration applied to each row as soon as its (w_i,u_i)
// exist.  w,u never reach memory; (r,s) are double-buffered (gathered from rs_old, written
// to rs_new); the 4 inner products ride along (partials[grid][0..4]).  Returns the grid.
// `prev`: if prev.nprev > 0 the inner products of the previous iteration are still block
// partials (prev.prev_partials[nprev][kPartialStride]); every block sums them itself in the
// fixed order and block 0 stores the result to prev.dots_prev_out -- no reduction launch
// between iterations.  Otherwise the reduced values are read from dots_prev.
int launch_pipe_fused(hipStream_t st, const CsrDev& A, const Tile* tiles, int ntiles, int steps,
                      const FusedState& f, TileKnobs kn = TileKnobs{});

// ---- window tiles: row-per-lane kernels for bands and stencils (prcg_win.hip) ---------------
// Planned on the host by plan_window_tiles (prcg_plan.cpp).  The CSR arrays are the caller's;
// device-internal, lossless re-encodings: cw8 / cw16[q] = index of col[q] in the tile's staged
// window of the input vector (page * 64 + offset); vidx8 / vdict = per-tile value dictionary
// (<= kWinDictMax distinct bit patterns per tile; entries ARE the caller's doubles).
struct WinDev {
    const int* indptr;
    const double* val;
    const unsigned char* cw8;      // geometry 0, 1
    const unsigned short* cw16;    // geometry 2, 3
    const unsigned char* vidx8;    // null: plain values
    const double* vdict;
    const unsigned short* rel;     // row pointers relative to the tile's first nonzero (tile.src_r); geometry 5: the rows' slot masks
    const PatRec* pat;             // geometry 5: the pattern records (tile.src_c = pattern id)
    int sweep_waves, sweep_tiles;  // geometry 5, sweep table (prcg_plan.h: plan_sweep_tiles): the waves / tiles the carry bits assume (0: none)
    int big_ok;                    // short launches of the one-launch iteration may take big workgroups (PRCG_WIN_BIG=0: never)
    int period;                    // > 1: tiles t and t + period read the same stream images (host: the launch picks a wave
                                   // count that is a multiple of it, so that a wave meets the same image tile after tile)
};
// same contracts as launch_spmv / launch_spmm2 / launch_pipe_fused below; per_cu > 0 overrides the
// number of workgroups launched per CU (experiments)
int launch_win_spmv(hipStream_t st, const WinDev& A, const WTile* tiles, int ntiles, int geom, const double* x, double* y,
                    SpmvEpilogue epi, const double* ep_r, const double* ep_d, double* ep_st, double* partials, int per_cu);
int launch_win_spmm2(hipStream_t st, const WinDev& A, const WTile* tiles, int ntiles, int geom, const double* rs, double* wu,
                     int write_mask, int per_cu, const StopAt& stop = StopAt{});      // (stop: as launch_spmm2)
int launch_win_pipe_fused(hipStream_t st, const WinDev& A, const WTile* tiles, int ntiles, int geom, const FusedState& f,
                          int per_cu);
// waves per workgroup the one-launch pipelined iteration WOULD take (prcg_debug_layout before any launch of a session; after
// one it reports win_last_launch, below)
int win_fused_waves_per_block(int geom, bool value_dict, bool deferred, int ntiles, bool big_ok, int sweep_waves);
// Workgroups and waves per workgroup of the calling thread's last window-tile launch, whichever launch_win_* issued it:
// recorded by launch_win_v from the WPB it instantiated and the grid it launched (the summation order of the launch's
// inner-product partials depends on both: prcg_debug_layout).  {0, 0}: none yet.
struct WinLaunchShape { int grid, wpb; };
WinLaunchShape win_last_launch();
// Second of the TWO launches of a Hestenes-Stiefel iteration on a window operator (hs_cg.py:57-61,
// hs_pcg :120-124).  The first (launch_hs_update_xr with `prev`) left nu_k = <r~,r> as block partials;
// every workgroup of this launch sums them in the same fixed order, b_k = nu_k / nu_k1, and the window of
// the input vector is FORMED while it is staged: p = z + b_k p_old (z = r, or r~ with Jacobi; mul then add,
// two roundings, as the reference's `r_k + b_k * p_k1`), so p_k is never gathered from memory.  Then
// s = A p with mu = <p,s> as block partials (partials[grid][0]); the row's own p goes to p_new (other
// tiles still stage p_old: double-buffered).  hs.prev_partials / nprev: the update launch's partials
// (slots 3, 4); hs.dots_old: scalars of iteration k-1; hs.dots_prev_out: scalars of iteration k (nu, rr
// written by workgroup 0); coef_out[1] = b_k.  nprev == 0: nu_k is read from dots_prev_out instead.
int launch_win_hs(hipStream_t st, const WinDev& A, const WTile* tiles, int ntiles, int geom, const double* z,
                  const double* p_old, double* p_new, double* s, double* partials, double* coef_out,
                  const FusedPrev& hs, int per_cu);
// ONE launch per iteration of the non-pipelined predict-and-recompute variants (pr_cg.py:146-158; pr_pcg, m_pcg) on
// a window operator.  These variants have ONE reduction per iteration, and everything the product needs from the
// update is a linear combination of old vectors with coefficients known at the head of the launch (a, b from the
// previous launch's partials -- predicted nu, pr_cg.py:149-150): the staged window of the new direction is FORMED
// while it is parked, p = (z - a zs) + b p_old (the reference's `rt_k1 - a_k1 * st_k1` then `rt_k + b_k * p_k1`:
// mul, sub, mul, add, four roundings), s = A p follows, and the row's own x, r, (r~), p, s, (s~) and the five
// inner-product partials mu = p.s, dl = r.s~, gm = s~.s, nu = r~.r, r.r are written by the lane that summed the row.
// f.pr: the vectors (see FusedPrev::PrOne; d null without Jacobi); f.prev_partials / nprev / dots_prev_out: as
// launch_pipe_fused; f.dots_old: the reduced scalars of iteration k-1 when nprev == 0; coef_out: a, b, predicted nu.
int launch_win_pr_one(hipStream_t st, const WinDev& A, const WTile* tiles, int ntiles, int geom, const FusedPrev& f,
                      int meurant, double* partials, double* coef_out, int per_cu);
// First of the TWO launches of a Chronopoulos-Gear iteration on a window operator (cg_cg.py:59-63, cg_pcg :116-121):
// a = nu_k1 / mu_k1 (f.dots_old), the staged window is the NEW residual formed while it is parked, r - a s (times d
// with Jacobi: r~ = M^-1 r), w = A r~ follows; the lane that summed row i writes x += a p, r (to f.pr.z_new: other
// tiles still stage the old r), r~ (f.pr.zs_new, Jacobi) and w, with the partials eta = w.r~ (slot 1), nu = r.r~ (3),
// r.r (4).  The second launch is launch_cg_update_ps with `prev`: it sums those partials in its prologue.
// f.pr: z_old = r, zs_old = s, p_old = p, z_new = the other r buffer, zs_new = r~ (Jacobi), x, d (Jacobi or null).
int launch_win_cg_w(hipStream_t st, const WinDev& A, const WTile* tiles, int ntiles, int geom, const FusedPrev& f,
                    double* w_out, double* partials, double* coef_out, int per_cu);
// The same for Ghysels-Vanroose (gv_cg.py:65-75, gv_pcg :152-164): the staged window is the new w formed as w - a u
// (times d: w~ = M^-1 w), t = A w~ follows; the lane that summed row i writes x += a p, r -= a s, (r~ -= a s~), w (to
// f.pr.z_new), (w~ to f.pr.zs_new), t, and the partials eta = w.r~ (1), nu = r.r~ (3), r.r (4).
// f.pr: z_old = w, zs_old = u, p_old = p, z_new = the other w buffer, zs_new = w~, x, r, s, d, rt, st.
int launch_win_gv_w(hipStream_t st, const WinDev& A, const WTile* tiles, int ntiles, int geom, const FusedPrev& f,
                    double* t_out, double* partials, double* coef_out, int per_cu);
// ONE launch per iteration of Chronopoulos-Gear (cg_cg.py:59-68, cg_pcg :116-137) or Ghysels-Vanroose (gv_cg.py:65-81,
// unpreconditioned).  Their reduction FOLLOWS the product it depends on, so an iteration cannot close inside its own
// launch -- but its tail can move into the next one: launch k+1 sums launch k's partials (nu_k, eta_k) in its prologue,
// derives b_k, mu_k = eta_k - (b_k / a_k1) nu_k and a_k = nu_k / mu_k, and applies the p, s (u) update of iteration k
// while it forms its window, which is the NEW vector of iteration k+1 expressed in old ones:
//   cg:  s_k = w + b s_old;  window  r_k1 = r - a (w + b s_old)   [times d];   w_k1 = A r~_k1
//   gv:  u_k = t + b u_old;  window  w_k1 = w - a (t + b u_old);               t_k1 = A w_k1
// (the reference's mul / add order: `w_k + b_k * s_k1` then `r_k1 - a_k1 * s_k1`).  The lane that summed row i writes
// x, p, (r, s), the three new buffers and the partials eta (slot 1), nu (3), r.r (4).  f.nprev == 0: p, s (u) are
// up to date (first launch of a call): no deferred update, a from f.dots_old = the complete scalars of the last
// iteration; else f.dots_old = the scalars of the iteration BEFORE the one whose partials are pending and
// f.dots_prev_out / f.lag.coef_prev receive that iteration's scalars and coefficients.  coef_out[0] = a.
int launch_win_cg_one(hipStream_t st, const WinDev& A, const WTile* tiles, int ntiles, int geom, const FusedPrev& f, int gv,
                      double* partials, double* coef_out, int per_cu);

// ---- sliced rows: lane-per-row kernels for medium-length rows (prcg_sell.hip) -----------------
// Planned on the host by plan_sell (prcg_plan.h): slices of up to 64 rows of one class; stored position u of the row in lane
// l at (u, l) of the slice -- val in chunks of two doubles, col16 in chunks of eight 16-bit column-DELTA codes (the lane's
// running column moves by code - 16384 per position; codes 0 / 65535 are skips: no nonzero) -- so that one wave
// instruction reads "positions u.. of all 64 rows" fully coalesced.  Lossless re-layout of the caller's CSR arrays.
// Slice descriptor: 8 int32 {first (smallest) row, that + rows, offset of the slice in val, offset in col16, longest stored
// row, smallest first column, first (row, stored length) pair in rows or -1, 0}.
struct SellDev {
    const int* indptr;
    const double* val;
    const unsigned short* col16;
    const int* rows;          // slices with rows_off >= 0 (a sorting window wider than a slice): (row, length) of lane l at pair rows_off + l (row -1: none)
    int nt;                   // 1: value / code streams read with nontemporal loads (operators far larger than the Infinity Cache)
    int run;                  // 1: a column code per nonzero; 3: a code per aligned run of three consecutive columns (prcg_plan.h)
    const int* gran;          // non-null: WINDOW codes (prcg_plan.h) -- the first column of every granule, slice after slice
    int window;               // ... and the most granules a slice has (<= 64)
};
int launch_sell_spmv(hipStream_t st, const SellDev& A, const void* slices, int nslices, const double* x, double* y, SpmvEpilogue epi,
                     const double* ep_r, const double* ep_d, double* ep_st, double* partials, int per_cu,
                     const StopAt& stop = StopAt{});      // (stop: as launch_spmv)
int launch_sell_spmm2(hipStream_t st, const SellDev& A, const void* slices, int nslices, const double* rs, double* wu, int write_mask,
                      int per_cu, const StopAt& stop = StopAt{});      // (stop: as launch_spmm2)
// [dst0 | dst1] = A [src0 | src1] for two pair arrays in ONE walk of the operator (four right-hand sides in one session): sources
// (n + g) x 2 with the spare entries of every product source, destinations n x 2; per column the bits of launch_sell_spmm2
// (stop: of a session whose columns stop (ProductStop): the same products, or nothing at all; stop.word is column 0's, the launch
//  reads column 1's behind it)
int launch_sell_spmm4(hipStream_t st, const SellDev& A, const void* slices, int nslices, const double* src0, const double* src1,
                      double* dst0, double* dst1, int per_cu, const StopAt& stop = StopAt{});
int launch_sell_pipe_fused(hipStream_t st, const SellDev& A, const void* slices, int nslices, const FusedState& f, int per_cu);
// New values on an unchanged pattern (prcg_update_values): sval, the re-laid value array A.val points to, rewritten from val_csr, the
// nnz values in the caller's CSR order -- one wave per slice, every position of a slice written (no nonzero: 0), so that sval holds
// the bytes plan_sell's fill pass would have produced from these values.  Reads A.indptr, A.rows and, for rows with skips, A.col16.
int launch_sell_set_values(hipStream_t st, const SellDev& A, const void* slices, int nslices, const double* val_csr, double* sval);

// ---- small systems: the whole solve in one launch of one workgroup (prcg_small.hip) -------------
struct SmallArgs {
    int n, nnz;
    const int* indptr; const int* col; const double* val;
    double* xp;        // pairs (x,p), read at entry, written at exit
    double* rs;        // pairs (r,s), read at entry, written at exit
    double* dots;      // [max_iter+1][kPartialStride]: row k0 is read, rows k0+1..k0+iters written
    double* coef;      // [max_iter+1][4]
    int k0, iters, meurant;
    double* hs_p; double* hs_s;   // launch_small_hs: xp = x, rs = r, and the direction and its product
};
// The fit rule: true and *mode = 1 (matrix in registers) or 0 (matrix in LDS beside the vectors); jacobi: the need of the bodies
// preconditioned by a diagonal scaling, which sum five inner products -- 128 B more LDS -- so a matrix in LDS may fit without
// the scaling and not with it (the mode of one that fits both ways is the same).  small_lds_bytes: the dynamic LDS of one system.
// prec: kSmallPrecNone, kSmallPrecJacobi (`jacobi` above) or kSmallPrecBlocks -- block Jacobi (SmallBlocks below), which needs
// what the scaling needs: its rows exchange through the buffer of the successor.
enum { kSmallPrecNone = 0, kSmallPrecJacobi = 1, kSmallPrecBlocks = 2 };
size_t small_lds_bytes(int n, int nnz, int mode, int prec = kSmallPrecNone);
bool small_fits(int64_t n, int64_t nnz, int max_row_len, int* mode, int prec = kSmallPrecNone);
// The single sessions.  The dynamic-LDS attribute of every kernel of the family is set, and its result checked, on first use on
// each device: a launch fails (-1) where it could not be set.
// stop (or null; SmallStop below): the single session stopped at a residual threshold -- the STOP form of the batch's body on the
// session's own word
int launch_small_pipe_pr(hipStream_t st, const SmallArgs& a, int mode, const SmallStop* stop = nullptr);
int launch_small_hs(hipStream_t st, const SmallArgs& a, int mode, const SmallStop* stop = nullptr);      // Hestenes-Stiefel, same storage
// ---- a batch of small systems: the same solver, one workgroup per system, blockIdx.x selects the system (prcg_batch.cpp) ----
// desc: `count` SmallArgs in DEVICE memory, all of one mode (k0, iters, meurant in them are ignored: the launch carries them).
// Results of a system are those of launch_small_pipe_pr / launch_small_hs with its descriptor, bit for bit, whatever its
// position or company in the launch.
// jac (or null): the batch preconditioned by a diagonal scaling d = inv_diag applied inside the one-workgroup solver.  What a
// Jacobi system holds beside its SmallArgs: the pairs (r~,s~) (pipelined only; read at entry, written at exit) and d.  jac[i]
// belongs to desc[i].  Pipelined: xp = (x,p), rs = (r,s), ts = (r~,s~); Hestenes-Stiefel: xp = x, rs = r, hs_p, hs_s, and r~ = d r
// is formed anew in every iteration.  dots[k] = {mu, delta, gamma, nu, rr} (HS: {mu, -, -, nu, rr}), nu = r~.r, rr = r.r.
struct SmallJacobi { double* ts; const double* d; };
// blk (or null; then jac is null): the batch preconditioned by point-block Jacobi applied inside the one-workgroup solver, blocks
// of 1..8 rows following a partition of the system.  blk[i] belongs to desc[i].  ts: as SmallJacobi's.  tab: one int2 per row,
// x = first row of the row's block | (size of the block << 16), y = offset of the row's row of the block's inverse in inv.  inv: the
// inverses, packed (block k: m_k x m_k row-major, no padding).  Row start + a forms (M^-1 v)_{start+a} = acc, acc = B[a][0] v[start],
// acc = acc + B[a][j] v[start+j] for j = 1 .. m-1, every product and sum rounded: the loop of k_bjvar_apply (prcg_blockjac.hip).
// The rows of a block exchange v through LDS, in the buffer of the successor: the pipelined body puts (w,u) there and writes the
// new (r~,s~) over the old, Hestenes-Stiefel puts r where the next direction goes.  Scalars and state as with jac.
struct SmallBlocks { double* ts; const int2* tab; const double* inv; };
// stop (or null): every system stopped at its OWN residual threshold, decided inside its workgroup.  stop[i] belongs to desc[i].
// thr: a bound on r.r, finite and >= 0.  word: two ints in device memory, word[0] the iteration the system stopped at (-1 while
// it runs), word[1] its status (0 running, 1 converged, 2 breakdown).  The rule, applied to row k of the scalars (mu = dots[k][0],
// nu = dots[k][3], rr = dots[k][4]) after iteration k, and to row 0 by the launch with k0 == 0:
//   rr <= thr -> converged;  else !(0 < mu < inf && 0 < nu < inf) -> breakdown (alpha = nu / mu is not an SPD system's);  else go on.
// A system stopped at k holds the complete state of iteration k: its vectors, scalar rows 0..k, coefficient rows 1..k; later
// rows are not written, and a later launch returns at once for it and stores nothing.  A system that never stops carries the
// bits of the launch without `stop`.
struct SmallStop { double thr; int* word; };
inline SmallStop StopAt::decides() const { return SmallStop{thr, word}; }
// one launch of a batch: the arrays above (device memory) and where the session stands
struct SmallBatchArgs { const SmallArgs* desc; const SmallJacobi* jac; const SmallStop* stop; int k0, iters, meurant; };
// lds: the largest small_lds_bytes(n, nnz, mode, prec) among the launch's systems -- each workgroup carves it by its own
// n and nnz.  blk: the block-Jacobi kernels (g.jac is ignored); they take it beside g, so the others keep their arguments
int launch_small_batch(hipStream_t st, const SmallBatchArgs& g, int count, int mode, size_t lds, bool hs, const SmallBlocks* blk = nullptr);
// x = x0, r = b - A x0, [r~ = d r,] p = r~, s = A p [, pipelined: s~ = d s] and row 0 of every system's scalars in ONE launch;
// init[i] belongs to desc[i]; jac null: no scaling (r~ is r); blk: r~ = M^-1 r and s~ = M^-1 s by the blocks (jac is ignored).  The vectors carry the bits of the single session's start-up
// launches; the inner products are summed in the order of the loop (thread-sequential rows, wave butterfly, 16 waves), not of
// those launches.
struct SmallInit { const double* b; const double* x0; };       // right-hand side and initial guess of one system
int launch_small_batch_init(hipStream_t st, const SmallArgs* desc, const SmallInit* init, const SmallJacobi* jac, int count, bool hs,
                            const SmallBlocks* blk = nullptr);

// ---- fused vector updates + inner products -----------------------------------------
struct PipeUpdateArgs {
    int64_t n;
    double* xp;       // pairs (x,p)
    double* rs;       // pairs (r,s)  -- when preconditioned: the plain pair, no ghosts
    double* rst;      // pairs (r~,s~) (preconditioned only; the SpMM input)
    double* wu;       // pairs (w,u)
    double* wt;       // w~ (preconditioned 'p' flavours only)
    const double* d;  // inverse diagonal (preconditioned only)
    const double* ut; // non-null: u~ = M^-1 u (and w~ in wt) were computed elsewhere (host-callback preconditioner)
    const double* dots_prev;   // kNumScalars doubles: mu, dl, gm, nu of iteration k-1
    double* coef_out;          // alpha, beta, nu_pred of this iteration
    double* partials;          // [grid][kPartialStride]
    int meurant;      // nu prediction flavour
    int recompute_w;  // 'pr' flavours: w is overwritten by the following SpMM
};
// stop: update stop.k of a STORED-TILDE session that stops at a threshold (prcg_set_stop_block_jacobi): the flavour with u~ and w~ as
// vectors only (a.ut set, a.d null; anything else: -1), a kernel of its own.  stop.word: the session's stop word ({iteration it
// stopped at or -1, status}: SmallStop's layout, written by launch_reduce_final's stop form on the same stream).  If 0 <= word[0] <
// stop.k the session stopped before this update and the launch returns at once: no load, no store, no coefficient row, no partial
// row, no barrier met.  Otherwise the statements of the launch without a stop in their order: the same bits in every vector and the
// same partial rows.  Returns the grid either way.
int launch_pipe_update(hipStream_t st, const PipeUpdateArgs& a, const StopAt& stop = StopAt{});
// the four (five) inner products of the current pipe state, no update (initialisation)
int launch_pipe_dots(hipStream_t st, const PipeUpdateArgs& a);

struct HsArgs {
    int64_t n;
    double* x; double* r; double* rt; double* p; const double* s; const double* d;
    const double* dots_prev; const double* dots_cur; double* coef_out; double* partials;
};
// prev_mu / nprev: mu = <p,s> of iteration k-1 still as block partials (slot 0) of the product launch -- every
// block sums them in the same fixed order and block 0 stores mu to dots_prev_w[0]; nprev == 0: a.dots_prev[0]
int launch_hs_update_xr(hipStream_t st, const HsArgs& a, const double* prev_mu = nullptr, int nprev = 0,
                        double* dots_prev_w = nullptr, const StopAt& stop = StopAt{});   // x,r,(rt); partial nu (slot 3), rr (slot 4)
// prev_nu / nprev: nu_k, rr_k still as block partials (slots 3, 4) of launch_hs_update_xr; block 0 stores them
// to dots_cur_w[3], [4]
int launch_hs_update_p(hipStream_t st, const HsArgs& a, const double* prev_nu = nullptr, int nprev = 0,
                       double* dots_cur_w = nullptr, const StopAt& stop = StopAt{});    // p = z + beta p
int launch_hs_init_dots(hipStream_t st, const HsArgs& a);   // nu, rr of the initial state
// stop: the launches of iteration k = stop.k of a Hestenes-Stiefel session that stops at a threshold (prcg_set_stop_hs), kernels of
// their own.  stop.word: the session's stop word, SmallStop's layout and rule.
//   update_xr (launch A of iteration k; k < 1: -1): returns at once if the session stopped before k - 1.  Otherwise mu_k1 as above
//     (workgroup 0 stores it: it belongs to the state of a stop), then the rule on row k - 1 = {mu_k1, nu_k1, rr_k1}, nu and rr read
//     from a.dots_prev, where the launch before stored them.  On a verdict thread 0 of workgroup 0 records {k - 1, status} and every
//     workgroup returns: no coefficient, no vector, no partial row of iteration k is written.  No verdict: the bits without a stop.
//   update_p (CSR-adaptive tiles and sliced rows): returns at once if the session stopped before k; else the bits without a stop.
//   launch_reduce_hs_mu (the reduction that ends a prcg_iterate call, and the session's start with k = 0): row[PRCG_S_MU] = mu_k,
//     one slot summed by launch_reduce_final.  With a stop it also DECIDES: it returns at once if the word is set (the partials
//     are stale); else the same sum, then the rule on {mu_k, row[3], row[4]} and the record {k, status}.
void launch_reduce_hs_mu(hipStream_t st, const double* partials, int nparts, double* row, const StopAt& stop = StopAt{});

// ---- Hestenes-Stiefel, TWO right-hand sides in one session (prcg_rhs2.hip; prcg_solve_begin_multi) ----
// x, r, rt, p, s: interleaved n x 2 arrays, row i = (column 0, column 1) -- p and s are directly the input and output of the
// two-vector product.  d: the inverse diagonal (n doubles, shared by both columns) or null.  The scalars of one iteration
// are ONE row of kPartialStride doubles holding both columns, the coefficients one row of four:
//   scalars  [mu_0, mu_1, -, nu_0, rr_0, nu_1, rr_1, -]        coefficients  [a_0, b_0, a_1, b_1]
// so that one launch_reduce_final serves both columns of a reduction (slots 0..1 of the product dot, 3..6 of the update).
constexpr int kHs2Mu = 0, kHs2Nu = 3, kHs2Rr = 4;      // slot of column c: kHs2Mu + c, kHs2Nu + 2 c, kHs2Rr + 2 c
struct Hs2Args {
    int64_t n;
    double* x; double* r; double* rt; double* p; const double* s; const double* d;
    const double* dots_prev; const double* dots_cur; double* coef_out; double* partials;
};
// every inner product of this session type is summed in the order of tests/device_order.py: device_sum (thread t of
// block b: elements (b * trips + j) * 512 + t, then + 256 + t, ascending j; butterfly; waves in order; launch_reduce_final)
int launch_hs2_update_xr(hipStream_t st, const Hs2Args& a);   // x, r, (rt); partials nu_c (slots 3, 5), rr_c (4, 6)
int launch_hs2_init_dots(hipStream_t st, const Hs2Args& a);   // ... of the initial state: no update, (rt = d r)
int launch_hs2_update_p(hipStream_t st, const Hs2Args& a);    // p = z + b_c p
int launch_hs2_dot_ps(hipStream_t st, const Hs2Args& a);      // partials mu_c = p.s (slots 0, 1)

// ---- predict-and-recompute (pr_pcg / m_pcg), TWO right-hand sides in one session (prcg_rhs2.hip) ----
// The interleaved n x 2 arrays of Hs2Args plus st (s~, with Jacobi).  Scalars and coefficients: TWO rows per iteration, row
// 2 k + c = column c's iteration k in the single-session order [mu dl gm nu rr - - -] / [a b nu_pred -], so that predict()
// reads a column's row as it reads a single session's.  dots_prev, coef_out: column 0's row (column 1's follows it).
// part0, part1: the block partials of column 0 / 1 in the same slots -- one launch_reduce_final per column sums all five.
constexpr int kPr2Mu = 0, kPr2Nu = 3;                  // slots: mu, dl, gm from the dots kernel; nu, rr from the update
constexpr int kPr2CoefStride = 4;                      // doubles per coefficient row (the engine's kCoefStride)
struct Pr2Args {
    int64_t n;
    double* x; double* r; double* rt; double* p; const double* s; double* st; const double* d;
    const double* dots_prev; double* coef_out; double* part0; double* part1;
    int meurant;
};
int launch_pr2_update(hipStream_t st, const Pr2Args& a);      // x, r, (rt), p; partials nu_c (slot 3), rr_c (4) of part[c]
// ... with r~ and s~ STORED vectors whatever `d` says (a.d is not read): r~ -= a s~ from rt, st.  The same kernel instantiation as
// launch_pr2_update with a diagonal; the block-Jacobi session selects it without one
int launch_pr2_update_stored(hipStream_t st, const Pr2Args& a);
int launch_pr2_init_dots(hipStream_t st, const Pr2Args& a);   // ... of the initial state: no update, (rt = d r)
int launch_pr2_dots(hipStream_t st, const Pr2Args& a);        // (st = d s); partials mu_c, dl_c, gm_c (slots 0..2) of part[c]

// ---- pipelined predict-and-recompute (pipe_pr_cg / pipe_pr_m_cg, with Jacobi pipe_pr_pcg / pipe_pr_m_pcg), TWO right-hand
// sides in one session (prcg_rhs2.hip; prcg_solve_begin_multi_pipe) ----
// Column c keeps the single session's 16-byte pairs: xp[c] = (x,p), rs[c] = (r,s), wu[c] = (w,u) and with Jacobi rst[c] =
// (r~,s~), n pairs each (rs[c] / rst[c], whichever feeds the product, with the spare entries of a product source).  d: the
// inverse diagonal shared by both columns, or null.  Scalars, coefficients and block partials: the layout of Pr2Args -- row
// 2 k + c = column c's iteration k, [mu dl gm nu rr - - -] / [a b nu_pred -]; dots_prev, coef_out: column 0's row; part0 /
// part1: five slots per block.  ONE launch updates both columns; wu is read only (the four-vector product rewrites it).
struct Pipe2Args {
    int64_t n;
    double* xp[2]; double* rs[2]; double* rst[2]; const double* wu[2]; const double* d;
    const double* dots_prev; double* coef_out; double* part0; double* part1;
    int meurant;
};
// stop: the update of a session whose columns stop at their own thresholds (prcg_set_stop_rhs).  stop.word: four ints in device
// memory, column c's stop word at word + 2 c ({iteration it stopped at or -1, status}: SmallStop's layout; written by
// launch_reduce_final's stop form).  A column whose word names an iteration is FROZEN: the launch loads and stores nothing of it --
// no vector, no coefficient row, no partial row (its reduction returns at once as well).  Both frozen: the launch returns in its
// prologue.  The other column carries the bits of the launch without a stop: the same expressions, accumulation order and tree.
int launch_pipe2_update(hipStream_t st, const Pipe2Args& a, const StopAt& stop = StopAt{});   // x, p, r, s, (r~, s~) of both columns; partials mu .. rr (slots 0..4) of part[c]
int launch_pipe2_dots(hipStream_t st, const Pipe2Args& a);     // the five sums of the state as it stands: no update (initialisation)

struct PrArgs {   // non-pipelined predict-and-recompute (pr_pcg / m_pcg)
    int64_t n;
    double* x; double* r; double* rt; double* p; const double* s; const double* st_;
    const double* dots_prev; double* coef_out; double* partials; int meurant; int precond;
};
int launch_pr_update(hipStream_t st, const PrArgs& a);      // x,r,rt,p; partial nu (3), rr (4)
int launch_pr_init_dots(hipStream_t st, const PrArgs& a);

struct CgArgs {   // Chronopoulos-Gear / Ghysels-Vanroose vector kernels
    int64_t n;
    double* x; double* r; double* rt; double* w; double* wt; double* p; double* s; double* st_; double* u;
    const double* t; const double* z;   // t = A w~ (gv); z = r~ or r
    const double* d;
    const double* dots_prev; const double* dots_cur; double* dots_cur_w; double* coef_out; double* partials;
};
// prev / nprev: eta, nu, r.r of this iteration still as block partials (slots 1, 3, 4) of launch_win_cg_w: every
// block sums them in the order of k_reduce_final, block 0 stores them to a.dots_cur_w
int launch_cg_update_ps(hipStream_t st, const CgArgs& a, const double* prev = nullptr, int nprev = 0);   // p,s,(s~),(u); mu by recurrence
int launch_gv_update1(hipStream_t st, const CgArgs& a, bool dots_only);   // x,r,(r~),w,(w~); partials eta(1), nu(3), rr(4)

// out[dst_first..+count) = fixed-order sum over blocks b of partials[b][src_first..+count).  0 / -1.
// stop (sessions with a threshold; (src_first, dst_first, count) = (0, 0, 5) only, anything else: -1 and nothing launched): the same
// kernel code, the same tree, the same bits in out[0..5) -- then the rule of SmallStop on {mu, nu, rr} = out[0], out[3], out[4], which
// are the scalars of iteration stop.k: a stop is recorded as {stop.k, status} in stop.word.  If the word is already set the launch
// returns at once and writes nothing: its partials belong to a launch that returned early.
int launch_reduce_final(hipStream_t st, const double* partials, int nparts, double* out,
                        int src_first, int dst_first, int count, const StopAt& stop = StopAt{});
// up to kMaxReduceJobs such reductions in ONE launch, one workgroup each: job j's result carries the bits of launch_reduce_final
// with its arguments (the same tree by the same code)
constexpr int kMaxReduceJobs = 4;
struct ReduceJob { const double* partials; int nparts; double* out; int src_first, dst_first, count; };
struct ReduceJobs { ReduceJob job[kMaxReduceJobs]; };
void launch_reduce_final_jobs(hipStream_t st, const ReduceJobs& jobs, int njobs);

// ---- small utility kernels (strided so they can address one half of a pair array) ----
void launch_copy(hipStream_t st, double* dst, int ds, const double* src, int ss, int64_t n);
void launch_sub(hipStream_t st, double* dst, int ds, const double* a, int as, const double* b, int bs, int64_t n);
void launch_mul(hipStream_t st, double* dst, int ds, const double* a, int as, const double* b, int bs, int64_t n);
// ---- point-block Jacobi (prcg_blockjac.hip): dst = blockdiag(B_k) src, uniform block size bs in 1..8 ----
// `blocks` is the DEVICE layout, not the caller's nb x bs x bs array: block_jacobi_layout re-lays it (entry j of the row
// of lane t of 256-lane tile T at (T * bs + j) * 256 + t: coalesced for a fixed j) and returns the number of doubles
// (out == nullptr: only that; -1 for bs outside 1..8).  Strides 1 or 2 (one column of a pair array).  0 / -1.
int64_t block_jacobi_layout(int64_t n, int bs, const double* inv_blocks, double* out);
int launch_block_jacobi(hipStream_t st, double* dst, int dstride, const double* src, int sstride, int64_t n, int bs, const double* blocks);
// the inverse of block_jacobi_layout on the host (prcg_get_block_jacobi): nb x bs x bs row-major from the device layout, a short
// last block as its leading m x m part inside an identity; returns the number of doubles written (-1 for bs outside 1..8)
int64_t block_jacobi_unlay(int64_t n, int bs, const double* laid, double* inv_blocks);
// the blocks built ON THE DEVICE from the caller-order CSR arrays (prcg_build_block_jacobi; contract in prcg.h): `blocks` receives
// the device layout (block_jacobi_layout's count of doubles, every one written), *first_bad (device, preset to INT64_MAX) the
// smallest index of a bad block.  0 / -1.
int launch_block_jacobi_build(hipStream_t st, double* blocks, int64_t n, int bs, const int* indptr, const int* col, const double* val,
                              long long* first_bad);
// both columns of the interleaved [w u] array in one launch: wt = M^-1 w (mask bit 0), ut = M^-1 u (mask bit 1)
// (stop: the pair launch of iteration stop.k of a session that stops at a threshold (ProductStop; prcg_set_stop_block_jacobi), a kernel
//  of its own: the pair launch belongs to the state of its iteration, so it runs unless the session stopped BEFORE stop.k
//  (0 <= stop.word[0] < stop.k: returns at once, nothing loaded or stored); otherwise the bits of the launch without a stop)
int launch_block_jacobi_pair(hipStream_t st, double* wt, double* ut, const double* wu, int64_t n, int bs, const double* blocks, int mask,
                             const StopAt& stop = StopAt{});
// ---- the same with VARIABLE block sizes (prcg_set_block_jacobi_var / prcg_build_block_jacobi_var): the partition reaches the
// kernels as prcg_bjvar.h's tables -- `tiles` ntiles x 4 int64 (first row, first line, first block, largest size), `code` and
// `bidx` one byte per lane, 256 per tile -- and `blocks` is that header's layout (BjVarPlan::doubles()).  0 / -1.
int launch_block_jacobi_var(hipStream_t st, double* dst, int dstride, const double* src, int sstride, int64_t ntiles, const long long* tiles,
                            const unsigned char* code, const double* blocks);
int launch_block_jacobi_var_pair(hipStream_t st, double* wt, double* ut, const double* wu, int64_t ntiles, const long long* tiles,
                                 const unsigned char* code, const double* blocks, int mask,
                                 const StopAt& stop = StopAt{});      // (stop: as launch_block_jacobi_pair)
// ---- M^-1 on an interleaved n x 2 array with the inner products that need the result, in ONE launch (block-Jacobi sessions with
// two or four right-hand sides: prcg_solve_begin_multi_block_jacobi).  v: the source pairs (NU: r; PR: s), z: the result (r~ / s~);
// p, r: read by PR only.  One partial row per TILE (a tile: 256 - 256 % bs rows, or a tile of the partition's table): part0 / part1
// hold block_jacobi_tiles(n, bs) (the partition's ntiles) rows of kPartialStride doubles.
//   kBjDotsNu: nu_c = r_c.z_c, rr_c = r_c.r_c -- part1 null: [nu_0 rr_0 nu_1 rr_1] in slots 3..6 of part0 (the Hs2Args scalar row);
//              else column c's two sums in slots 3, 4 of part[c] (the Pr2Args slots)
//   kBjDotsPr: mu_c = p_c.s_c, dl_c = r_c.z_c, gm_c = z_c.s_c in slots 0..2 of part[c]
// The launchers return the grid (= the number of partial rows written), -1 on failure.
enum { kBjDotsNu = 0, kBjDotsPr = 1 };
struct BjDotsArgs {
    int64_t n;
    const double* v; double* z; const double* p; const double* r;
    double* part0; double* part1;
};
int64_t block_jacobi_tiles(int64_t n, int bs);
int launch_block_jacobi_dots(hipStream_t st, int mode, const BjDotsArgs& a, int bs, const double* blocks);
int launch_block_jacobi_var_dots(hipStream_t st, int mode, const BjDotsArgs& a, int64_t ntiles, const long long* tiles,
                                 const unsigned char* code, const double* blocks);
// gather, invert, store: every double of the layout is written; *first_bad as in launch_block_jacobi_build
int launch_block_jacobi_var_build(hipStream_t st, double* blocks, int64_t ntiles, const long long* tiles, const unsigned char* code,
                                  const unsigned char* bidx, const int* indptr, const int* col, const double* val, long long* first_bad);
// partial[slot] = sum (a[i*as] - b[i])^2
int launch_diff_sq(hipStream_t st, const double* a, int as, const double* b, int64_t n, double* partials, int slot);
// partial[slot] = sum a_i * b_i
int launch_dot(hipStream_t st, const double* a, const double* b, int64_t n, double* partials, int slot);
// buf[j*nc + c] = v[idx[j]*nc + c]
void launch_pack(hipStream_t st, double* buf, const double* v, const int* idx, int64_t count, int nc);
// merged exchange for small halos: see k_gather_pack / k_gather_unpack
void launch_gather_pack(hipStream_t st, const double* partials, int nparts, double* slot, const double* rs,
                        const int* send_idx, int nsend);
void launch_gather_unpack(hipStream_t st, const double* gbuf, int slot_doubles, int nranks, double* dots_out,
                          double* rs_ghost, const int* ghost_src, int nghost, double* pub = nullptr, unsigned pub_value = 0,
                          hipEvent_t done = nullptr);
// peer exchange outside the iteration launches (session start, teacher forcing): send this rank's rows of `rs` to the
// neighbours' ghost areas of parity k & 1 and its slot for iteration k (contribute: the slot carries dots, else zeros --
// the engine lets rank 0 alone contribute the GLOBAL inner products of the state just set: the sum in rank order is
// then exactly that)
void launch_peer_push(hipStream_t st, const PeerDev* px, const double* rs, const double* dots, int k, int contribute);
// one wave: if nparts > 0 first adds this rank's block partials of iteration k (lane l: rows l, l + 64, ...; butterfly --
// as the communication wave of the next launch would) and sends the slot; then waits (bounded) until all ranks' slots
// of iteration k have arrived, adds them in rank order into dots_out[0..5) and, if pub, publishes them with counter
// k; *err = 1 on a timeout
void launch_peer_collect(hipStream_t st, const PeerDev* px, int k, const double* partials, int nparts, double* dots_out, double* pub,
                         unsigned* err);
// marks the window tiles that own rows of the send plan (bit 30 of WTile::geo)
void launch_flag_send_tiles(hipStream_t st, void* wtiles, const void* tile_send, int ntiles);
// every copy c: pub[8c .. 8c+5) = dots[0..5), then the copy's counter (byte 48 of the record) = value: what the
// deferred one-launch iteration waits for
constexpr int kPubCopies = 64;
constexpr int kPubDoubles = 8 * kPubCopies;
void launch_publish(hipStream_t st, const double* dots, double* pub, unsigned value);
// one launch of the streaming probes (prcg_stream_ceiling): mode 0 reads a[0..n_pairs) pairs; 1 / 2: a read and rewritten,
// b read, c written (plain / nontemporal stores)
void launch_stream_mix(hipStream_t st, const double* v, double* x, const double* r, double* rn, size_t n_rows, int kb);
void launch_stream_probe(hipStream_t st, int mode, double* a, double* b, double* c, size_t n_pairs);
// one wave on `st` waits (bounded, ~2 ms) for the record to reach `want`; *err = 1 if it does not
void launch_probe_wait(hipStream_t st, const double* pub, unsigned want, unsigned* err);

}  // namespace prcg
