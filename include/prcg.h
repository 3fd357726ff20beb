/*
 * prcg.h -- C-ABI of libprcg.so: predict-and-recompute CG on AMD MI355X (gfx950).
 *
 * The reference (tchen-research/new_cg_variants) has no FFI layer: its hot path is
 * reached through two Python call signatures,
 *
 *   trial  = method(A, b, x0, max_iter, callbacks=..., x_true=..., preconditioner=...)
 *            numerical_experiments/figure_gen.py:59   (solvers: cg_variants/hs_cg.py:9,
 *            cg_variants/pipe_pr_cg.py:9-105,109-216, cg_variants/pr_cg.py:93-176)
 *   sol, t = variant(comm, A, b, max_iter)
 *            scaling_experiments_mpi4py/scaling_tests.py:71 (cg_variants/pipe_pr_cg.py:7,
 *            cg_variants/hs_cg.py:7)
 *
 * and everything below them is SciPy/NumPy/BLAS/MPI.  This header is the boundary a
 * maintainer binds instead (ctypes stub: INTEGRATION.md): plain pointers and sizes,
 * no Python or torch types.  One handle = one GPU = one rank (one process per GPU);
 * the caller owns every host buffer before and after each call, the library owns
 * all device memory, streams and the RCCL communicator.
 *
 * Return value: 0 on success, otherwise one of PRCG_E*; text via prcg_last_error().
 * Numerical breakdown is NOT an error: inf/nan land in the histories exactly as in
 * the reference (which never raises; figure_gen.py:89 uses nanmin).
 * A handle is not re-entrant; distinct handles may be used from distinct threads.
 */
#ifndef PRCG_H
#define PRCG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct prcg_handle prcg_t;

/* ---- error classes --------------------------------------------------------- */
#define PRCG_OK       0
#define PRCG_EINVAL   1   /* bad argument / call order                     */
#define PRCG_EHIP     2   /* HIP runtime error (no GPU, OOM, launch fault) */
#define PRCG_ERCCL    3   /* RCCL could not be loaded or returned an error */
#define PRCG_ENOMEM   4   /* host allocation failed                        */

/* ---- variants: which recurrence prcg_solve_begin sets up --------------------
 * names = the reference's function names, numerical_experiments/cg_variants/__init__.py:64-74 */
#define PRCG_HS          0  /* hs_cg / hs_pcg            hs_cg.py:9,70               */
#define PRCG_PIPE_PR     1  /* pipe_pr_cg / pipe_pr_pcg  pipe_pr_cg.py:89,201        */
#define PRCG_PIPE_P      2  /* pipe_p_cg / pipe_p_pcg    pipe_pr_cg.py:83,195        */
#define PRCG_PIPE_PR_M   3  /* pipe_pr_m_cg / _pcg       pipe_pr_cg.py:101,213       */
#define PRCG_PIPE_P_M    4  /* pipe_p_m_cg / _pcg        pipe_pr_cg.py:95,207        */
#define PRCG_PR          5  /* pr_pcg                    pr_cg.py:166                */
#define PRCG_M           6  /* m_pcg                     pr_cg.py:172                */
#define PRCG_CG_CG       7  /* cg_cg / cg_pcg  (Chronopoulos-Gear)   cg_cg.py:9,76      */
#define PRCG_GV          8  /* gv_cg / gv_pcg  (Ghysels-Vanroose)    gv_cg.py:9,93      */
#define PRCG_NUM_VARIANTS 9

/* ---- history recorders (bit mask), = the four callbacks of figure_gen.py:37 ---- */
#define PRCG_HIST_UPDATED_RESIDUAL_2_NORM  1u  /* callbacks/updated_residual_2_norm.py:40 */
#define PRCG_HIST_RESIDUAL_2_NORM          2u  /* callbacks/residual_2_norm.py:41         */
#define PRCG_HIST_ERROR_A_NORM             4u  /* callbacks/error_A_norm.py:47-48         */
#define PRCG_HIST_ERROR_2_NORM             8u  /* callbacks/error_2_norm.py:47-48         */
#define PRCG_HIST_ALL                     15u

/* ---- state vectors addressable by prcg_get_vector / prcg_set_vector ---------
 * (the reference's x_k, r_k, p_k, s_k, w_k, u_k and the tilde companions) */
#define PRCG_VEC_X   0
#define PRCG_VEC_R   1
#define PRCG_VEC_P   2
#define PRCG_VEC_S   3
#define PRCG_VEC_W   4
#define PRCG_VEC_U   5
#define PRCG_VEC_RT  6
#define PRCG_VEC_ST  7
#define PRCG_VEC_WT  8
#define PRCG_VEC_UT  9
#define PRCG_NUM_VECS 10

/* ---- per-iteration scalars (one row of prcg_get_scalars) ---------------------- */
#define PRCG_S_MU     0   /* p.s                                   */
#define PRCG_S_DELTA  1   /* r.s~   (cg_cg / gv: eta = w.r~)        */
#define PRCG_S_GAMMA  2   /* s~.s                                  */
#define PRCG_S_NU     3   /* r~.r                                  */
#define PRCG_S_RR     4   /* r.r   (= nu when unpreconditioned)    */
#define PRCG_S_RES2   5   /* |b - A x|^2        if recorded        */
#define PRCG_S_ERRA2  6   /* e'Ae, e = x-x_true if recorded        */
#define PRCG_S_ERR2   7   /* |e|^2              if recorded        */
#define PRCG_NUM_SCALARS 8

typedef struct prcg_timings {
    double tot_ms;          /* wall time of the last prcg_solve loop (host clock, synced) */
    double iter_ms;         /* tot_ms / iterations                                        */
    double spmv_ms;         /* mean device time of the SpMV/SpMM launch (HIP events)      */
    double update_ms;       /* mean device time of the fused vector-update launch         */
    int64_t spmv_samples;   /* number of launches spmv_ms averages over                   */
    int64_t iterations;     /* iterations timed                                           */
} prcg_timings;

/* ---- life cycle -------------------------------------------------------------- */
int  prcg_create(prcg_t** h, int device_id);
void prcg_destroy(prcg_t* h);
/* h may be NULL: text of the last error of a failed prcg_create / prcg_comm_unique_id */
const char* prcg_last_error(const prcg_t* h);
/* ABI version of this header */
int  prcg_version(void);

/* Experiment switches (the PRCG_* names of INTEGRATION.md, e.g. "PRCG_FUSED" = "0"): prcg_create
 * takes their defaults from the environment, this call sets one for ONE handle -- before
 * prcg_set_csr, which fixes the operator's encodings.  No counterpart in the reference. */
int prcg_set_option(prcg_t* h, const char* key, const char* value);

/* ---- multi-GPU: one RCCL communicator per handle --------------------------------
 * replaces comm = MPI.COMM_WORLD (scaling_tests.py:21) for the data path.
 * rccl_path: path of the librccl.so to dlopen (NULL -> "librccl.so.1").  Rank 0
 * calls prcg_comm_unique_id (once per id) and ships the 128-byte ids to the other
 * ranks by any means (torch.distributed in bench.py); then every rank calls
 * prcg_comm_init with n_ids = 1 or 2 consecutive ids.  With 1 id the neighbour exchange
 * and the all-reduce of an iteration form one chain on the communication stream; with 2
 * ids the halo exchange gets a communicator and a stream of its own and the two run
 * side by side. */
int prcg_comm_unique_id(const char* rccl_path, void* id128);
int prcg_comm_init(prcg_t* h, const char* rccl_path, int rank, int nranks, const void* ids, int n_ids);

/* Ghysels-Vanroose residual replacement (gv_cg.py:9,69-71; gv_pcg :93,156-158): `w_replace(k=..., x=..., w=..., r=..., ...)`
 * is the CALLER's predicate.  fn(ctx, k) is called inside prcg_iterate of a PRCG_GV session after x, r, (r~), w of
 * iteration k are updated and before t = A w~; it may read the state with prcg_get_vector (x, r, w are the new ones, p, s, u
 * the old ones -- what the reference passes); a non-zero return replaces w by A r (r, not r~, also with a preconditioner, as
 * the reference does) before the iteration goes on.  Sessions with a hook run the unfused schedule on one stream. */
typedef int (*prcg_replace_fn)(void* ctx, int k);
int prcg_set_replace_hook(prcg_t* h, prcg_replace_fn fn, void* ctx);

/* ---- direct peer exchange over xGMI ----------------------------------------------------
 * The reduction and the halo of the pipelined loop WITHOUT a collective (replaces, inside the loop, the
 * `comm.Allreduce` of scaling_experiments_mpi4py/cg_variants/pipe_pr_cg.py:67 and the neighbour exchange its dense
 * column blocks make implicit): every rank owns one exchange buffer in fine-grained device memory, mapped into every
 * other rank's process (hipIpc); the iteration launch stores the rows its neighbours need and its five partial inner
 * products straight into their buffers, and waits inside the kernel for theirs.  One host call
 * per iteration, no communication stream.  Call after prcg_set_csr / prcg_set_halo, on EVERY rank or on none:
 *   prcg_peer_setup    allocates this rank's buffer for `max_ghost_any_rank` ghost rows (the largest ghost count of any
 *                      rank: every buffer has the same layout), returns its 64-byte hipIpcMemHandle and, for ranks that
 *                      share the process (tests: ranks in threads), its device address;
 *   prcg_peer_connect  ipc_handles: nranks x 64 bytes, rank order (own entry ignored), or same_process_ptrs[q] non-null
 *                      for a rank of this process; send_dst_off[q]: where in peer q's ghost area (prcg_set_halo's
 *                      receive order of THAT rank) this rank's rows for it begin.
 * Window operators only (others keep the RCCL schedule); PRCG_PEER=0 turns it off.  Waits are bounded: a rank that
 * waits ~10 s for another sets an error that prcg_sync and the next prcg_iterate report. */
int prcg_peer_setup(prcg_t* h, int64_t max_ghost_any_rank, void* ipc_handle64, void** local_ptr);
int prcg_peer_connect(prcg_t* h, const void* ipc_handles, void* const* same_process_ptrs, const int64_t* send_dst_off);
/* ---- operator -------------------------------------------------------------------
 * The rank's row block in CSR (what `A` is in figure_gen.py:350 / scaling_tests.py:51),
 * column indices already LOCAL: [0,n_rows) = owned entries, [n_rows, n_rows+n_ghost)
 * = ghost entries received from peers, in the order fixed by prcg_set_halo.
 * indptr: int32 or int64 (indptr_is64), n_rows+1 entries; nnz < 2^31.  Indices need
 * not be sorted, but the sequential per-row summation order of SciPy's csr_matvec is
 * reproduced only in the order given.  Copies to the device and builds the
 * CSR-adaptive tile tables (interior rows / rows that touch ghosts). */
int prcg_set_csr(prcg_t* h, int64_t n_rows, int64_t n_ghost, int64_t nnz,
                 const void* indptr, int indptr_is64,
                 const int32_t* indices, const double* data);

/* New values for the nonzeros of the operator set by prcg_set_csr: same n_rows, nnz, indptr, indices (the caller's
 * promise -- nothing of the pattern is passed again), data[q] replaces the value of nonzero q in that CSR order.
 * data_on_device = 0: nnz host doubles.  data_on_device = 1: nnz doubles in device memory of the handle's GPU
 * (e.g. a torch tensor's data_ptr(); the caller has synchronised whatever wrote them).
 * Replaces a second prcg_set_csr (a second DeviceCSR(A)) with the same pattern -- the same mesh with new coefficients: Newton
 * steps, a time-dependent material, a re-assembled stiffness matrix -- and with it the reference's re-assignment of `A`
 * between calls of `method(A, b, x0, max_iter, ...)` (figure_gen.py:59), which there costs nothing because scipy streams the
 * CSR arrays as they are.  Which of two routes serves the call depends on the encodings prcg_set_csr chose (prcg_values_route):
 *   0, in place: no encoding of the operator holds values (no value dictionary, no pattern tiles).  The handle keeps its plan --
 *      family, tiles, slices, column codes, grids, hence the summation tree of every inner product; the values are copied into
 *      the caller-order value array on the compute stream once the handle's pending work has finished, and for sliced rows
 *      one kernel re-lays them (k_sell_set_values).  No host planning; nothing else is touched.  The handle does NOT decide
 *      again: an operator whose new values would qualify for a value dictionary keeps plain values until the next prcg_set_csr.
 *   1, re-planned: result and state are those of prcg_set_csr with the new values under the handle's options (the row pointers
 *      and column indices are read back from the device, no host copy of them is kept) -- a dictionary may fall to plain values,
 *      pattern tiles to index streams, and back.
 * On both routes an open session ends (as after prcg_set_csr) while the session buffers stay allocated; options, a
 * host-callback preconditioner and block-Jacobi blocks stay in force (a frozen preconditioner is legitimate; call
 * prcg_build_block_jacobi or prcg_set_block_jacobi for new blocks).  The call returns after `data` has been read -- the caller may overwrite it -- though
 * the re-lay kernel may still be enqueued.  nnz == 0: nothing to do.
 * Refused (PRCG_EINVAL, the text names the reason, the handle is untouched): no operator; null data with nnz > 0; n_ghost > 0,
 * a communicator or a world size > 1 on the handle (rank-local blocks: set them again with prcg_set_csr); data_on_device
 * outside 0 / 1; a device pointer the runtime does not report as device memory of the handle's GPU, or with
 * [data, data + nnz) leaving its allocation -- the library reads no pointer it has not checked. */
int prcg_update_values(prcg_t* h, const double* data, int data_on_device);
/* how prcg_update_values serves the operator now on the handle: 0 = in place (no host planning), 1 = re-planned;
 * -1 without an operator */
int prcg_values_route(const prcg_t* h);

/* Halo plan (needed iff n_ghost > 0).  Peer q = peer_rank[q]:
 *   send_idx[send_ptr[q] .. send_ptr[q+1])  local rows whose entries peer q needs
 *   ghost slots [recv_ptr[q], recv_ptr[q+1]) receive from peer q, in the peer's send order. */
int prcg_set_halo(prcg_t* h, int n_peers, const int32_t* peer_rank,
                  const int64_t* send_ptr, const int32_t* send_idx,
                  const int64_t* recv_ptr);

/* y = A x on the device, `reps` times (x: n_rows host doubles; ghosts exchanged when
 * n_ghost > 0).  ms_avg (nullable) = mean device time per launch by HIP events.
 * Replaces `A @ v` -> scipy _sparsetools.csr_matvec (hs_cg.py:23,26,59). */
int prcg_spmv(prcg_t* h, const double* x, double* y, int reps, double* ms_avg);
/* y = A_local [x_own ; x_ghost]: the row block's product with the ghost entries supplied by the
 * caller (n_rows + n_ghost host doubles) instead of by a halo exchange -- no communicator needed.
 * Runs the interior launch and the boundary launch of the overlapped schedule.  What one rank of
 * `A @ v` computes once its halo has arrived (scaling_experiments_mpi4py/cg_variants/hs_cg.py:49-51). */
int prcg_spmv_ext(prcg_t* h, const double* x_ext, double* y);
/* [w u] = A [r s], the fused two-vector product of the pipelined loop
 * (pipe_pr_cg.py:69-70; mpi4py pipe_pr_cg.py:65).  rs, wu: n_rows x 2 row-major. */
int prcg_spmm2(prcg_t* h, const double* rs, double* wu, int reps, double* ms_avg);
/* [y_0 y_1 y_2 y_3] = A [x_0 x_1 x_2 x_3], the product of a four-RHS session (prcg_solve_begin_multi with nrhs = 4), on the
 * route that session takes: ONE launch that reads the operator once on sliced-row operators (PRCG_SPMM4=0: never), two
 * two-vector launches (columns 0, 1 and 2, 3) on every other operator -- per column the bits of prcg_spmm2 either way.
 * Replaces four `A @ v` (hs_cg.py:23,26,59 for each of four right-hand sides).  x4, y4: n_rows x 4 row-major host doubles.
 * Single GPU, n_ghost == 0. */
int prcg_spmm4(prcg_t* h, const double* x4, double* y4, int reps, double* ms_avg);

/* ---- solver session ----------------------------------------------------------------
 * begin: upload b, x0 (+ optional x_true, inv_diag), run the variant's initialisation
 *        (hs_cg.py:22-28 / pipe_pr_cg.py:22-36,122-140 / pr_cg.py:106-116) and record
 *        history index 0.  max_iter as in the reference: histories have max_iter
 *        entries, index 0 = initial state, at most max_iter-1 iterations follow.
 *        inv_diag != NULL selects the Jacobi-preconditioned recurrences with
 *        z = inv_diag * r (figure_gen.py:43); NULL = the unpreconditioned ones.
 * iterate: enqueue `iters` iterations on the device; returns without waiting.
 * sync: wait for everything enqueued. */
int prcg_solve_begin(prcg_t* h, int variant, const double* b, const double* x0,
                     int max_iter, const double* x_true, const double* inv_diag,
                     uint32_t hist_mask);
int prcg_iterate(prcg_t* h, int iters);
int prcg_sync(prcg_t* h);
/* current iteration index k (0 after begin) */
int prcg_iteration(const prcg_t* h);
/* which schedule the current session runs (valid after prcg_solve_begin): bit 0 one launch per
 * iteration (fused SpMM + update), bit 1 one-workgroup solver, bit 2 communicator present,
 * bit 3 merged exchange (halo rows ride on the one all-gather that carries the partial inner
 * products), bit 4 second halo communicator, bits 5..7 the operator's stream encodings (valid after
 * prcg_set_csr); bits 8..11 tile size in 256-slot steps.
 * No counterpart in the reference (diagnostics for tests and benchmarks). */
#define PRCG_SCHED_FUSED 1
#define PRCG_SCHED_SMALL 2
#define PRCG_SCHED_COMM 4
#define PRCG_SCHED_GATHER 8
#define PRCG_SCHED_DUAL_COMM 16
#define PRCG_SCHED_VALDICT 32   /* interior tiles stream 1-byte value-dictionary indices (lossless) */
#define PRCG_SCHED_COL8 64      /* ... and 1-byte tile-relative column offsets */
#define PRCG_SCHED_COL16 128    /* ... 2-byte */
#define PRCG_SCHED_FUSED_COMM 8192 /* one launch per iteration WITH a communicator: the interior launch waits in-kernel
                                      for the reduced inner products of the previous iteration */
#define PRCG_SCHED_SELL 32768  /* lane-per-row kernels over 64-row slices (medium-length rows: assembled FEM matrices) */
#define PRCG_SCHED_PEER 16384  /* ... through the direct peer exchange (prcg_peer_setup / prcg_peer_connect): no collective in the loop */
#define PRCG_SCHED_PATTERN 65536 /* ... window kernels over PATTERN tiles (constant-coefficient stencils): no per-nonzero stream at all --
                                    per tile one pattern record (slot offsets + values) and the rows' 16-bit slot masks */
#define PRCG_SCHED_STREAM_STORES 131072 /* the one-launch iteration writes its row results with nontemporal stores (vectors far larger than the caches) */
#define PRCG_SCHED_SELL_SORTED 262144  /* sliced rows with a sorting window wider than a slice (SELL-C-sigma: row lengths vary) */
#define PRCG_SCHED_NT_LOADS 524288     /* sliced rows: value / column-code streams read with nontemporal loads (operator far larger than the Infinity Cache) */
#define PRCG_SCHED_SELL_WINDOW 2097152 /* sliced rows with WINDOW codes: a slice's input entries staged in LDS, per nonzero an LDS read instead of a gather */
#define PRCG_SCHED_BLOCK_JACOBI 4194304 /* stored-tilde schedule with M^-1 applied by the block-Jacobi kernel (prcg_set_block_jacobi) */
#define PRCG_SCHED_XP_DEFERRED 8388608 /* single-GPU one-launch pipelined iteration: prcg_iterate runs its launches in pairs, the first of a
                                          pair does not store (x,p) and the second rebuilds them bit for bit (PRCG_XP_DEFER=0: off) */
#define PRCG_SCHED_RHS2 16777216 /* the session solves TWO right-hand sides (prcg_solve_begin_multi): one two-vector product per iteration */
#define PRCG_SCHED_RHS4 33554432 /* the session solves FOUR right-hand sides as two pair groups (PRCG_SCHED_RHS2 means exactly two: clear here) */
#define PRCG_SCHED_SPMM4 67108864 /* ... and its product is ONE four-vector launch (sliced rows; else two two-vector launches) */
#define PRCG_SCHED_RHS2_PIPE 134217728 /* the two-RHS session is the PIPELINED one (prcg_solve_begin_multi_pipe): PRCG_SCHED_RHS2 is set too, and
                                       * PRCG_SCHED_SPMM4 says whether its product of four vectors is one launch */
/* 1048576: retired (was PRCG_SCHED_MEDIUM, the few-workgroup solver of mid-size systems); never to be reused */
#define PRCG_SCHED_WINDOW 4096  /* row-per-lane window kernels (bands, stencils): the column stream holds indices into the tile's
                                   LDS-staged window of the input vector */
/* A preconditioner that is not a diagonal scaling: `fn(ctx, n, v, out)` must write M^-1 v to out (host buffers,
 * n doubles each; return 0).  It stands for the `preconditioner` callable of the reference's *_pcg functions
 * (numerical_experiments/cg_variants/hs_cg.py:70, pr_cg.py:93, pipe_pr_cg.py:109, cg_cg.py:74, gv_cg.py:87), which
 * is the caller's code there too.  Sessions begun with inv_diag == NULL while a function is set call it wherever
 * the reference calls `preconditioner(...)`: the vector goes to the host, the result comes back -- two PCIe copies
 * and a stream synchronisation per application (1 per iteration for hs / cg_cg / gv / pr / m and the 'p' pipelined
 * flavours, 2 for the 'pr' pipelined flavours), on the schedules in which every tilde vector is a stored vector.
 * Single GPU.  fn == NULL removes it.  Jacobi stays on the device: pass inv_diag to prcg_solve_begin instead. */
typedef int (*prcg_prec_fn)(void* ctx, int64_t n, const double* v, double* out);
int prcg_set_preconditioner(prcg_t* h, prcg_prec_fn fn, void* ctx);
/* Point-block Jacobi ON THE DEVICE: M^-1 = blockdiag(B_0 .. B_{nb-1}), one uniform block size bs in 1..8, the step after
 * scalar Jacobi for assembled FEM matrices with bs unknowns per node.  No counterpart in the reference (its only
 * preconditioner is the Jacobi lambda, figure_gen.py:43); the counterpart elsewhere is PETSc's `-pc_type pbjacobi`.
 * Rows k*bs .. k*bs+bs-1 form block k, nb = ceil(n_rows / bs); inv_blocks: nb x bs x bs host doubles, row-major, the
 * INVERSES of the diagonal blocks (the caller inverts them); a short last block (m = n_rows - bs*(nb-1) < bs rows) uses
 * its leading m x m part, the rest is ignored.  Row i = k*bs + a of the result is
 *     acc = B[k][a][0] * v[k*bs];   acc = acc + B[k][a][j] * v[k*bs + j]   for j = 1 .. columns-1, ascending,
 * every product and every sum rounded (no FMA): the bits of the same loop on the host.
 * Call after prcg_set_csr (which fixes n_rows; a later prcg_set_csr drops the blocks); the blocks are copied to the device.
 * Sessions begun with inv_diag == NULL while blocks are set run the schedules of a host-callback session (every tilde
 * vector a stored vector) with one kernel launch on the compute stream where that session calls fn: no copy, no
 * synchronisation; the pipelined variants apply it to w and u in one launch.  inv_diag != NULL still selects Jacobi.
 * This call and prcg_set_preconditioner replace each other: the last one set is in force.  Single GPU.
 * inv_blocks == NULL removes it. */
int prcg_set_block_jacobi(prcg_t* h, int bs, const double* inv_blocks);
/* The same blocks BUILT ON THE DEVICE from the operator now on the handle: one kernel pass over the caller-order CSR arrays the
 * handle keeps (current after prcg_update_values on both routes) gathers the bs x bs diagonal blocks, inverts them and stores
 * them where the apply kernel reads them -- no host pass over the matrix, no upload.  No counterpart in the reference; it
 * replaces the caller's own gather-and-invert in front of prcg_set_block_jacobi (cg_variants.BlockJacobi: a NumPy pass over
 * every nonzero plus LAPACK), which a Newton loop would otherwise pay beside every prcg_update_values.
 * The arithmetic is fixed, so that a host restatement (cg_variants.invert_blocks) has the same bits:
 *   gather   rows k*bs .. k*bs+bs-1 form block k, nb = ceil(n_rows / bs).  Row i = k*bs + a starts with g[c] = +0.0, c < bs; for
 *            q = indptr[i] .. indptr[i+1]-1 ascending: if indices[q] / bs == k then g[indices[q] % bs] = g[indices[q] % bs] +
 *            data[q].  Unsorted rows and duplicates are legal; duplicates add in CSR order.  A short last block (m = n_rows -
 *            bs*(nb-1) < bs rows) is its leading m x m part inside an identity.
 *   invert   Gauss-Jordan on [M | E], E = I, NO pivoting (CG needs an SPD operator, whose diagonal blocks are SPD).  For c = 0 ..
 *            bs-1:  p = M[c][c];  row c becomes M[c][j] / p and E[c][j] / p for every j (a division, not a multiplication by a
 *            reciprocal);  for every r != c:  f = M[r][c];  M[r][j] = M[r][j] - f * M[c][j],  E[r][j] = E[r][j] - f * E[c][j] for
 *            every j.  Every quotient, product and difference rounded (no FMA).  E is the inverse.
 *   bad      a block is bad iff one of its pivots is zero or not finite at its step, or an entry of its E is not finite.  A block
 *            that is not bad carries exactly the bits of this loop, signed zeros included.  (A block such as [[0,1],[1,0]] is bad
 *            here although it has an inverse.)
 * Call after prcg_set_csr; valid again after every prcg_update_values.  The call waits for the handle's pending work, drops
 * blocks set before, runs the kernel on the compute stream and reads the flag back.  On success the state is that of
 * prcg_set_block_jacobi with these inverses (sessions, PRCG_SCHED_BLOCK_JACOBI, the mutual replacement with
 * prcg_set_preconditioner; a later prcg_set_csr drops them, a later prcg_update_values leaves them frozen) and *first_bad_block
 * (nullable) = -1.  With a bad block: PRCG_EINVAL, text "diagonal block K (bs = B) is singular or not finite", K the smallest
 * index of a bad block, *first_bad_block = K, and the handle is left WITHOUT blocks.
 * Refused (PRCG_EINVAL, the text names the reason, the handle is untouched): no operator; bs outside 1..8; n_ghost > 0; a
 * communicator or a world size > 1 on the handle. */
int prcg_build_block_jacobi(prcg_t* h, int bs, int64_t* first_bad_block);
/* The blocks now on the handle, whichever call set them: inv_blocks receives nb x bs x bs host doubles, row-major (bs: the one
 * they were set with); a short last block comes back as its leading m x m part inside an identity.  PRCG_EINVAL without blocks. */
int prcg_get_block_jacobi(prcg_t* h, double* inv_blocks);
/* Point-block Jacobi with VARIABLE block sizes, applied and built on the device: the blocks follow the nodes of a mesh whose nodes
 * carry different numbers of unknowns (shells next to solids, constrained nodes, mixed elements), where no uniform bs lines up.
 * No counterpart in the reference; the counterpart elsewhere is PETSc's `-pc_type vpbjacobi`, next to pbjacobi above.
 *   partition  block_ptr: nb + 1 int64 host entries, block_ptr[0] == 0, block_ptr[nb] == n_rows, every size
 *              m_k = block_ptr[k+1] - block_ptr[k] in 1..8.  Block k owns rows -- and the same columns -- block_ptr[k] .. block_ptr[k+1]-1.
 *   packed     inv_blocks holds block k as m_k x m_k doubles, row-major, at offset sum of m_q^2 over q < k: no padding, no identity fill.
 *   apply      row i = block_ptr[k] + a of the result is
 *                  acc = B_k[a][0] * v[block_ptr[k]];   acc = acc + B_k[a][j] * v[block_ptr[k] + j]   for j = 1 .. m_k-1, ascending,
 *              every product and every sum rounded (no FMA) -- word for word the loop of prcg_set_block_jacobi, so that on a uniform
 *              partition (a short last block included) the result has the bits of prcg_set_block_jacobi with the same inverses.
 *   build      gather: row i of block k starts with g[c] = +0.0, c < m_k; for q = indptr[i] .. indptr[i+1]-1 ascending: if
 *              block_ptr[k] <= indices[q] < block_ptr[k+1] then g[indices[q] - block_ptr[k]] = g[...] + data[q].  Unsorted rows and
 *              duplicates are legal; duplicates add in CSR order.  invert: the Gauss-Jordan loop of prcg_build_block_jacobi on the
 *              m_k x m_k block for exactly m_k steps -- no pivoting, the pivot row divided (not multiplied by a reciprocal), every
 *              other row one product and one difference per entry.  (The uniform build of a short last block, padded with an identity
 *              and run for bs steps, leaves exactly these bits in its leading m x m part: a uniform partition gives the uniform
 *              build's bits.)  bad: as there -- a pivot zero or not finite at its step, or an entry of E not finite.
 * State and life cycle are those of the uniform calls: call after prcg_set_csr; a later prcg_set_csr drops the blocks, a later
 * prcg_update_values leaves them frozen; prcg_set_block_jacobi, prcg_build_block_jacobi, these two setters and
 * prcg_set_preconditioner replace each other, the last one is in force; inv_blocks == NULL in the setter removes the blocks.
 * Sessions begun with inv_diag == NULL while variable blocks are set run the stored-tilde schedule exactly as a uniform block-Jacobi
 * session does, with the variable kernels where M^-1 is applied (one vector, or the pair [w u] of the pipelined variants in one
 * launch); prcg_schedule reports PRCG_SCHED_BLOCK_JACOBI | PRCG_SCHED_BLOCK_JACOBI_VAR.  The multi-RHS sessions refuse them as
 * they refuse uniform blocks.  The partition is cut into tiles on the host in O(nb); the matrix is never touched there.
 * Refused (PRCG_EINVAL, the text names the reason, the handle is untouched -- blocks set before stay in force): no operator; null
 * block_ptr; block_ptr[0] != 0 or block_ptr[nb] != n_rows; a size outside 1..8 (the text names the first such block and its size);
 * for the build also n_ghost > 0, a communicator or a world size > 1.
 * prcg_build_block_jacobi_var with a bad block: PRCG_EINVAL, text "diagonal block K (size M) is singular or not finite", K the
 * smallest such index, *first_bad_block = K (nullable; -1 otherwise), and the handle is left WITHOUT blocks.
 * prcg_get_block_jacobi_var returns the blocks now on the handle in the packed format; it refuses while the blocks on the handle
 * are uniform (use prcg_get_block_jacobi), as prcg_get_block_jacobi refuses while they are variable. */
int prcg_set_block_jacobi_var(prcg_t* h, int64_t nb, const int64_t* block_ptr, const double* inv_blocks);
int prcg_build_block_jacobi_var(prcg_t* h, int64_t nb, const int64_t* block_ptr, int64_t* first_bad_block);
int prcg_get_block_jacobi_var(prcg_t* h, double* inv_blocks);   /* packed, as above */
#define PRCG_SCHED_BLOCK_JACOBI_VAR 268435456   /* set together with PRCG_SCHED_BLOCK_JACOBI: the blocks have variable sizes */
int prcg_schedule(const prcg_t* h);
/* Bytes of the operator AS THE DEVICE STREAMS IT (the lossless re-encodings of the caller's CSR built at
 * prcg_set_csr: narrow column / window indices, value-dictionary indices, relative row pointers, tile
 * descriptors; stream images that many tiles share are counted once): what one matrix product must read
 * from memory at least once.  bench.py's roofline is computed from this figure plus the vector traffic
 * (SURVEY.md section 8d gives the algorithmic figure for the caller's CSR: 12 B per nonzero + 4 B per row).
 * -1 without an operator.  No counterpart in the reference (scipy streams the CSR arrays as they are). */
int64_t prcg_operator_bytes(const prcg_t* h);
/* teacher forcing: declare that the state now loaded (prcg_set_vector / prcg_set_scalars
 * for iteration k) IS iteration k; the next prcg_iterate(h,1) produces k+1 */
int prcg_set_iteration(prcg_t* h, int k);

/* state access (synchronises first); vectors are n_rows host doubles */
int prcg_get_vector(prcg_t* h, int which, double* out);
int prcg_set_vector(prcg_t* h, int which, const double* in);
/* scalars of iteration k: PRCG_NUM_SCALARS doubles */
int prcg_get_scalars(prcg_t* h, int k, double* out);
int prcg_set_scalars(prcg_t* h, int k, const double* in);
/* coefficients used BY iteration k (k>=1): out[0]=alpha (a_k1), out[1]=beta (b_k),
 * out[2]=predicted nu */
int prcg_get_coefficients(prcg_t* h, int k, double* out);

/* histories: for each bit set in hist_mask (ascending bit order) max_iter doubles;
 * entries beyond the current iteration are 0, as numpy.zeros(max_iter) leaves them. */
int prcg_get_history(prcg_t* h, double* hist);
/* ---- Hestenes-Stiefel or predict-and-recompute with TWO right-hand sides in one session (or FOUR) --------
 * Replaces TWO calls of the reference's hs_cg (numerical_experiments/cg_variants/hs_cg.py:9) or hs_pcg (:70), of pr_pcg
 * (pr_cg.py:166) or of m_pcg (pr_cg.py:172) on one matrix: load cases, time steps with a frozen operator, columns of a
 * block solve.  The two recurrences stay what they are
 * -- each column has its own a_k, b_k, inner products and history, nothing of one column enters the other (a breakdown of
 * one leaves the other's bits untouched) -- but every iteration streams the operator ONCE: s = A p of both columns is one
 * two-vector product (what prcg_spmm2 runs), on assembled FEM matrices most of an iteration's memory traffic.
 *   variant: PRCG_HS, PRCG_PR or PRCG_M.  nrhs: 2 or 4.  b, x0: nrhs pointers to n_rows host doubles each.  inv_diag != NULL:
 *   hs_pcg / pr_pcg / m_pcg with Jacobi, the same diagonal for both columns; inv_diag == NULL: hs_cg, or for PRCG_PR / PRCG_M
 *   the identity-preconditioned recurrences (this library's pr_cg / m_cg).  hist_mask: 0 or PRCG_HIST_UPDATED_RESIDUAL_2_NORM.
 *   A Hestenes-Stiefel iteration is six launches around its two dependent inner products; a predict-and-recompute
 *   iteration has ONE reduction point: update, two-vector product, the inner products that need s, one reduction per column.
 * Single GPU, whole operators: refused (PRCG_EINVAL, text names the reason) with a communicator on the handle, n_ghost > 0,
 * a host-callback or block-Jacobi preconditioner or a replace hook set, another variant, nrhs, or history bit.
 * prcg_iterate / prcg_sync / prcg_iteration / prcg_set_profiling / prcg_get_timings serve the session as they are.  State is
 * read per column j = 0, 1 with the calls below; the single-column accessors (prcg_get_vector, prcg_set_vector,
 * prcg_get_scalars, prcg_set_scalars, prcg_get_coefficients, prcg_get_history, prcg_set_iteration) are refused while it
 * is open.  A later prcg_solve_begin on the handle opens an ordinary session again.
 * Every inner product is summed in one fixed order: results are reproducible bit for bit, and
 * exchanging the two right-hand sides exchanges the two results bit for bit.
 * nrhs = 4 (replaces FOUR calls of the reference's function): two PAIR GROUPS, columns (0, 1) and (2, 3), each a complete
 * two-RHS state with its own vectors, inner products and coefficients, iterated by the same vector kernels around ONE product
 * [S_0 S_1 | S_2 S_3] = A [P_0 P_1 | P_2 P_3] (what prcg_spmm4 runs; PRCG_SCHED_SPMM4 says whether it is one launch).  Columns
 * (0, 1) and (2, 3) carry the bits of two two-RHS sessions begun with those pairs; the accessors below take j = 0 .. 3 and
 * return per column what they return in a two-RHS session; the refusals are those of the two-RHS session, word for word. */
int prcg_solve_begin_multi(prcg_t* h, int variant, int nrhs, const double* const* b, const double* const* x0,
                           int max_iter, const double* inv_diag, uint32_t hist_mask);
/* ---- pipelined predict-and-recompute with TWO right-hand sides in one session --------------------------------------------
 * Replaces TWO calls of the reference's pipe_pr_cg (numerical_experiments/cg_variants/pipe_pr_cg.py:89) or pipe_pr_pcg (:201),
 * of pipe_pr_m_cg (:101) or of pipe_pr_m_pcg (:213) on one matrix.  The pipelined iteration needs [w u] = A [r s] per system;
 * for two systems that is ONE product of four vectors, [w_0 u_0 | w_1 u_1] = A [r_0 s_0 | r_1 s_1] (what prcg_spmm4 runs: one
 * launch on sliced-row operators, PRCG_SCHED_SPMM4; else two two-vector launches, the same bits), so every iteration streams
 * the operator ONCE for both systems.  Each column keeps the single session's state -- the pairs (x,p), (r,s), (w,u) and with
 * Jacobi (r~,s~); w~ = d w and u~ = d u are formed in registers -- its own a_k, b_k, predicted nu, inner products and history;
 * nothing of one column enters the other.  An iteration is three steps: one update launch for both columns, one reduction
 * launch per column, the product.
 *   variant: PRCG_PIPE_PR or PRCG_PIPE_PR_M (the flavours that recompute w).  nrhs: 2.  b, x0: two pointers to n_rows host
 *   doubles each.  inv_diag != NULL: pipe_pr_pcg / pipe_pr_m_pcg with Jacobi, the same diagonal for both columns.  hist_mask: 0
 *   or PRCG_HIST_UPDATED_RESIDUAL_2_NORM.
 * A new entry, not a case of prcg_solve_begin_multi (which keeps refusing the pipelined variants).  Refused (PRCG_EINVAL, the
 * text names the reason; an open session stays as it was): PRCG_PIPE_P / PRCG_PIPE_P_M (the stored-w flavours) and every other
 * variant, nrhs != 2 (an eight-vector product does not exist), a communicator on the handle, n_ghost > 0, a host-callback or
 * block-Jacobi preconditioner or a replace hook set, another history bit, null b or x0.
 * prcg_iterate / prcg_sync / prcg_iteration / prcg_set_profiling / prcg_get_timings serve the session as they are; prcg_schedule
 * reports PRCG_SCHED_RHS2 | PRCG_SCHED_RHS2_PIPE.  State is read per column j = 0, 1 with the calls below -- vectors PRCG_VEC_X,
 * _R, _P, _S, _W, _U, with Jacobi _RT and _ST; _WT and _UT are refused (never stored); scalars mu, delta, gamma, nu, rr;
 * coefficients alpha, beta, the predicted nu -- and the single-column accessors are refused while it is open.  A later
 * prcg_solve_begin or prcg_solve_begin_multi opens an ordinary session again.  Every inner product is summed in one fixed
 * order: exchanging the two right-hand sides exchanges the two results bit for bit. */
int prcg_solve_begin_multi_pipe(prcg_t* h, int variant, int nrhs, const double* const* b, const double* const* x0,
                                int max_iter, const double* inv_diag, uint32_t hist_mask);
/* ---- TWO or FOUR right-hand sides preconditioned by POINT-BLOCK JACOBI, in one session -----------------------------------
 * Replaces two (four) calls of the reference's hs_pcg (hs_cg.py:70), pr_pcg (pr_cg.py:166) or m_pcg (pr_cg.py:172) on one matrix
 * with `preconditioner` the point-block Jacobi IN FORCE ON THE HANDLE: the blocks prcg_set_block_jacobi, prcg_build_block_jacobi,
 * prcg_set_block_jacobi_var or prcg_build_block_jacobi_var put there.  (A Newton loop: prcg_update_values, prcg_build_block_jacobi,
 * this call.)  The blocks stay on the handle afterwards as after a single session; a later prcg_set_csr drops them, a later
 * prcg_update_values leaves them frozen.
 *   variant: PRCG_HS, PRCG_PR or PRCG_M.  nrhs: 2 or 4 (two pair groups: columns (0, 1) and (2, 3) carry the bits of two two-RHS
 *   block sessions begun with those pairs, around ONE product of both groups' directions, PRCG_SCHED_SPMM4 as above).  b, x0: nrhs
 *   pointers to n_rows host doubles each.  hist_mask: 0 or PRCG_HIST_UPDATED_RESIDUAL_2_NORM.
 * State per pair group: the interleaved n x 2 arrays X, R, P, S of prcg_solve_begin_multi, r~ a STORED vector and, for PRCG_PR /
 * PRCG_M, s~ too.  M^-1 v is, word for word, the loop of prcg_set_block_jacobi / _var (acc = B[a][0] * v[start]; acc = acc +
 * B[a][j] * v[start + j] for ascending j, every product and sum rounded), applied to both columns in one launch that reads every
 * block once and leaves, in the same launch, the partial sums of the inner products that need the result:
 *   Hestenes-Stiefel  r~ = M^-1 r is formed anew in every iteration: update (x, r), BLOCK launch (r~; nu = r.r~, rr = r.r),
 *                     reduction, p = r~ + b p, product, mu = p.s (the vector launch of prcg_solve_begin_multi), reduction;
 *   PRCG_PR / PRCG_M  r~ is recurred (r~ -= a s~), s~ = M^-1 s is applied once per iteration: update (x, r, r~, p; nu, rr from this
 *                     vector launch), product, BLOCK launch (s~; mu = p.s, delta = r.s~, gamma = s~.s), ONE reduction launch for the
 *                     five sums of both columns.  At the start nu and rr come from a block launch as well (r~ = M^-1 r).
 * Every inner product is summed in one fixed order that depends on n and the partition only (the sums of a
 * block launch by tile -- lane t the row tile_row0 + t, butterfly, waves in order, tiles in order through the final tree).  Each
 * column has its own scalars; nothing of one column enters another; exchanging the right-hand sides exchanges the results bit
 * for bit; a NaN stays in its column.
 * A new entry: prcg_solve_begin_multi and prcg_solve_begin_multi_pipe keep refusing a handle with blocks set.  Refused here
 * (PRCG_EINVAL, the text names the reason; the handle and an open session stay as they were): no operator, no blocks on the handle,
 * another variant (the pipelined ones: a follow-up), nrhs outside {2, 4}, a communicator, n_ghost > 0, a replace hook, another
 * history bit, null b or x0, max_iter < 1.
 * prcg_iterate / prcg_sync / prcg_iteration / prcg_set_profiling / prcg_get_timings serve the session as they are; prcg_schedule
 * reports PRCG_SCHED_RHS2 or PRCG_SCHED_RHS4, PRCG_SCHED_BLOCK_JACOBI (| PRCG_SCHED_BLOCK_JACOBI_VAR for a partition) and
 * PRCG_SCHED_SPMM4 where it applies.  State is read per column with the calls below: vectors PRCG_VEC_X, _R, _P, _S, _RT, for
 * PRCG_PR / PRCG_M also _ST; scalars {mu, -, -, nu, rr} (PRCG_PR / PRCG_M: {mu, delta, gamma, nu, rr}); the single-column
 * accessors are refused while it is open.  A later prcg_solve_begin* opens an ordinary session. */
int prcg_solve_begin_multi_block_jacobi(prcg_t* h, int variant, int nrhs, const double* const* b, const double* const* x0,
                                        int max_iter, uint32_t hist_mask);
/* which: PRCG_VEC_X, _R, _P, _S (and _RT with Jacobi or block Jacobi; PRCG_PR / PRCG_M sessions with either also _ST; pipelined
 * sessions: see prcg_solve_begin_multi_pipe); out: n_rows host doubles */
int prcg_get_vector_rhs(prcg_t* h, int which, int j, double* out);
/* PRCG_NUM_SCALARS doubles: mu, nu, rr of column j at iteration k in their slots (PRCG_PR / PRCG_M sessions: mu, delta,
 * gamma, nu, rr; pipelined sessions the same), every other slot 0 */
int prcg_get_scalars_rhs(prcg_t* h, int k, int j, double* out);
/* out[0] = alpha, out[1] = beta used BY iteration k (k >= 1) of column j; out[2] = the predicted nu of iteration k in a
 * PRCG_PR / PRCG_M session, 0 in a Hestenes-Stiefel session (which predicts none) */
int prcg_get_coefficients_rhs(prcg_t* h, int k, int j, double* out);
/* max_iter doubles: column j's updated_residual_2_norm history (nothing is written when hist_mask was 0) */
int prcg_get_history_rhs(prcg_t* h, int j, double* hist);

/* ---- a single PIPELINED session stopped at a residual threshold, decided on the device ------------------------------------
 *   prcg_set_stop      rr_stop: NULL clears the threshold; else *rr_stop is a threshold on r.r (for a tolerance tol on the 2-norm
 *                      of the updated residual: tol * tol), finite and >= 0, else PRCG_EINVAL (the threshold set before stays).
 *                      It is copied at the call and applies to single sessions BEGUN afterwards with prcg_solve_begin (signature
 *                      unchanged); an open session is not affected.  Such a session stops by itself, decided on the device without
 *                      the host: after iteration k, and at k = 0 on the initial state, on row k of its scalars, mu = [0], nu = [3],
 *                      rr = [PRCG_S_RR], by the rule of prcg_batch_set_stop below, in this order:
 *                        1. rr <= *rr_stop                                     -> stop, status 1 (converged);
 *                        2. else !(0 < mu && mu < inf && 0 < nu && nu < inf)   -> stop, status 2 (breakdown);
 *                        3. else go on (status 0, stop iteration -1).
 *                      A session stopped at k keeps the complete state of iteration k: x, r, p, s, w, u (with Jacobi r~, s~ too;
 *                      the 'p' flavours their stored w and w~) are those of iteration k, scalar rows 0..k and coefficient rows 1..k
 *                      are written; prcg_get_scalars / prcg_get_coefficients of later rows and later entries of every history
 *                      read as zero.  The launches prcg_iterate had enqueued beyond the stop return at once and store nothing;
 *                      prcg_sync resolves the stop -- after it prcg_iteration reports k -- and prcg_iterate on a stopped session
 *                      is a no-op that returns PRCG_OK.  A threshold of 0 stops on an exactly zero residual (b = A x0) and on
 *                      breakdown only.  A session that never stops carries the bits of a session without a threshold.
 *                      Served while a threshold is set: the four pipelined variants (PRCG_PIPE_PR, PRCG_PIPE_PR_M, PRCG_PIPE_P,
 *                      PRCG_PIPE_P_M) on one GPU, unpreconditioned or with inv_diag, on the one-launch schedule or the
 *                      one-workgroup solver.  prcg_solve_begin refuses everything else (PRCG_EINVAL, the text says what is served)
 *                      -- another variant, a communicator or ghost rows, a host-callback or block-Jacobi preconditioner in force
 *                      (the stored-tilde schedule), PRCG_FUSED=0, a replace hook -- and nothing falls back to a schedule that
 *                      cannot stop.  In a session begun with a threshold prcg_set_vector, prcg_set_scalars and prcg_set_iteration
 *                      are refused.  Sessions with several right-hand sides ignore the threshold; the pipelined two-RHS session
 *                      stops each column at a threshold of its own (prcg_set_stop_rhs below), the others cannot stop.
 *   prcg_get_stop      synchronises; *k_stop, *status of the open single session: the iteration it stopped at and why (1 converged,
 *                      2 breakdown), or -1 and 0 while it runs -- and for a session begun without a threshold.  Refused without an
 *                      open single session. */
int prcg_set_stop(prcg_t* h, const double* rr_stop);
int prcg_get_stop(prcg_t* h, int32_t* k_stop, int32_t* status);

/* ---- a single pipelined session WITH POINT-BLOCK JACOBI stopped at a residual threshold, decided on the device ----------------
 * Blocks pay off in iteration counts, so this is the session whose max_iter is hardest to guess.  It runs the stored-tilde
 * schedule (an update launch, the product, one launch that applies the blocks to w and u), which prcg_set_stop does not serve:
 * it has a setter of its own, and every launch of an iteration a stop form of its own.
 *   prcg_set_stop_block_jacobi  rr_stop: NULL clears the threshold; else *rr_stop is the threshold on r.r, finite and >= 0, else
 *                      PRCG_EINVAL (what was set before stays).  It is copied at the call and applies to sessions BEGUN afterwards
 *                      with prcg_solve_begin; an open session is not affected.  While it is set prcg_solve_begin serves PRCG_PIPE_PR,
 *                      PRCG_PIPE_PR_M, PRCG_PIPE_P and PRCG_PIPE_P_M on one GPU with uniform or variable blocks in force
 *                      (prcg_set_block_jacobi / prcg_set_block_jacobi_var, or built on the device), and refuses everything else
 *                      with PRCG_EINVAL and a text that names this setter and how to clear it: another variant, no blocks in force
 *                      (such a session stops through prcg_set_stop), an inv_diag argument (it overrides the blocks), a host-callback
 *                      preconditioner, a communicator or ghost rows, a replace hook; prcg_solve_begin_multi,
 *                      prcg_solve_begin_multi_pipe and prcg_solve_begin_multi_block_jacobi refuse as well.  Nothing falls back to a
 *                      session that cannot stop.  Independent of prcg_set_stop: with both set, that setter's refusal of a session
 *                      with blocks stands.  The rule is prcg_set_stop's, on row k of the scalars after iteration k and on row 0:
 *                        1. rr <= *rr_stop                                     -> stop, status 1 (converged);
 *                        2. else !(0 < mu && mu < inf && 0 < nu && nu < inf)   -> stop, status 2 (breakdown);
 *                        3. else go on.
 *                      Iteration k is: update k (skipped if the session stopped at k - 1 or earlier); the reduction that sums row
 *                      k and applies the rule; the product and the block launch of k, which belong to the state of k and are
 *                      skipped only if the session stopped BEFORE k.  A session stopped at k therefore holds the complete state of
 *                      iteration k -- x, r, p, s, w, u, r~, s~, u~, w~, scalar rows 0..k, coefficient rows 1..k -- and every later
 *                      launch returns at once and writes nothing.  A session that does not stop carries the bits of the session
 *                      without a threshold; a session begun without one launches the kernels it always did.  prcg_sync resolves the
 *                      stop and prcg_get_stop reads it; afterwards prcg_iteration is k, prcg_iterate is a no-op, scalar and
 *                      coefficient rows and history entries beyond k read as zero.  prcg_set_vector, prcg_set_scalars and
 *                      prcg_set_iteration are refused in such a session; recorders are allowed as with prcg_set_stop.  The
 *                      one-workgroup solver is never taken: a session with blocks runs this schedule whatever n. */
int prcg_set_stop_block_jacobi(prcg_t* h, const double* rr_stop);

/* ---- a single HESTENES-STIEFEL session stopped at a residual threshold, decided on the device -----------------------------------
 * hs_cg / hs_pcg is the method a user reaches for first, and the session whose max_iter had to be guessed longest.  Its iteration has
 * two dependent reductions and no launch that holds all of a row's scalars at once, which prcg_set_stop does not serve: it has a
 * setter of its own, and every launch of an iteration a stop form of its own.
 *   prcg_set_stop_hs   rr_stop: NULL clears the threshold; else *rr_stop is the threshold on r.r, finite and >= 0, else PRCG_EINVAL
 *                      (what was set before stays).  It is copied at the call and applies to sessions BEGUN afterwards with
 *                      prcg_solve_begin; an open session is not affected.  While it is set prcg_solve_begin serves PRCG_HS on one
 *                      GPU, unpreconditioned or with inv_diag, on the schedule without reduction launches or on the one-workgroup
 *                      solver, and refuses everything else with PRCG_EINVAL and a text that names this setter and how to clear it:
 *                      another variant, a communicator or ghost rows, a host-callback or block-Jacobi preconditioner in force (the
 *                      stored-tilde schedule with reduction launches), PRCG_FUSED=0, a replace hook; prcg_solve_begin_multi,
 *                      prcg_solve_begin_multi_pipe and prcg_solve_begin_multi_block_jacobi refuse as well.  Nothing falls back to a
 *                      session that cannot stop.  Independent of prcg_set_stop and prcg_set_stop_block_jacobi: with one of those set,
 *                      its own refusal of PRCG_HS stands.  The rule is prcg_set_stop's, on row k of the scalars after iteration k
 *                      and on row 0; a Hestenes-Stiefel row is {mu_k = p_k.s_k, -, -, nu_k = r~_k.r_k, rr_k}:
 *                        1. rr <= *rr_stop                                     -> stop, status 1 (converged);
 *                        2. else !(0 < mu && mu < inf && 0 < nu && nu < inf)   -> stop, status 2 (breakdown);
 *                        3. else go on.
 *                      It is what a system of a Hestenes-Stiefel batch applies (prcg_batch_set_stop): a system in a batch and a
 *                      single session stop at the same k on the same bits.  Iteration k is: the update of x, r (r~), whose prologue
 *                      completes row k - 1 with mu and applies the rule to it (skipped, like everything after it, if that stops
 *                      the session at k - 1); the update of p and the product s = A p with the partial sums of mu_k, which decide
 *                      nothing and are skipped only if the session stopped BEFORE k.  The reduction that ends a prcg_iterate call
 *                      completes and decides the last row.  A session stopped at k therefore holds the complete state of iteration
 *                      k -- x, r, p, s (with inv_diag r~ too), scalar rows 0..k, coefficient rows 1..k -- and every later launch
 *                      returns at once and writes nothing.  The product s_k = A p_k of the stop iteration is computed although rr_k
 *                      is known before it: one product per solve, the price of one rule for every session type.  A session that
 *                      does not stop carries the bits of the session without a threshold; a session begun without one launches the
 *                      kernels it always did.  prcg_sync resolves the stop and prcg_get_stop reads it; afterwards prcg_iteration
 *                      is k, prcg_iterate is a no-op, scalar and coefficient rows and history entries beyond k read as zero.
 *                      prcg_set_vector, prcg_set_scalars and prcg_set_iteration are refused in such a session; recorders are
 *                      allowed as with prcg_set_stop. */
int prcg_set_stop_hs(prcg_t* h, const double* rr_stop);

/* ---- each column of a PIPELINED TWO-RHS session stopped at its own residual threshold, decided on the device ------------------
 * Two load cases of one matrix almost never converge at the same iteration: the session freezes the column that is done and
 * keeps iterating the other.
 *   prcg_set_stop_rhs  rr_stop: NULL clears the thresholds (nrhs is then not looked at); else nrhs thresholds on r.r, rr_stop[c]
 *                      column c's, each finite and >= 0, else PRCG_EINVAL naming the column (what was set before stays).  nrhs
 *                      must be 2: only the pipelined two-RHS session can stop.  The thresholds are copied at the call and apply
 *                      to sessions BEGUN afterwards with prcg_solve_begin_multi_pipe (signature unchanged); an open session is
 *                      not affected.  They are independent of prcg_set_stop: single sessions ignore these thresholds as multi-RHS
 *                      sessions ignore that one.  While they are set prcg_solve_begin_multi and
 *                      prcg_solve_begin_multi_block_jacobi refuse (PRCG_EINVAL; the text says what is served and that
 *                      prcg_set_stop_rhs(h, 0, NULL) clears): nothing falls back to a session that cannot stop.
 *                      The rule is prcg_set_stop's, applied to column c's OWN row k of scalars after iteration k, and at k = 0 on
 *                      the initial state:
 *                        1. rr <= rr_stop[c]                                   -> stop, status 1 (converged);
 *                        2. else !(0 < mu && mu < inf && 0 < nu && nu < inf)   -> stop, status 2 (breakdown);
 *                        3. else go on (status 0, stop iteration -1).
 *                      A column stopped at k_c keeps the complete state of iteration k_c -- x, r, p, s, w, u, with Jacobi r~, s~ --
 *                      its scalar rows 0..k_c and coefficient rows 1..k_c are written, and its later rows and later history entries
 *                      read as zero through prcg_get_scalars_rhs, prcg_get_coefficients_rhs and prcg_get_history_rhs.  The other
 *                      column runs on unaffected: from the stop onward it carries, bit for bit, what it carries in a session
 *                      without thresholds, and a column that never stops carries those bits throughout.  A threshold of 0 stops on
 *                      an exactly zero residual or on breakdown only.  prcg_sync resolves the stops.  Once BOTH columns have
 *                      stopped prcg_iteration reports max(k_0, k_1) and prcg_iterate is a no-op returning PRCG_OK; while a column
 *                      still runs prcg_iteration counts what was launched.  prcg_get_stop keeps refusing multi-RHS sessions, and
 *                      they keep having no setters.
 *   prcg_get_stops_rhs synchronises; k_stop[c], status[c] of every column of the open multi-RHS session: the iteration it stopped
 *                      at and why (1 converged, 2 breakdown), or -1 and 0 for a column that still runs -- and for every column of a
 *                      session begun without thresholds.  Refused without an open multi-RHS session and with a null buffer. */
int prcg_set_stop_rhs(prcg_t* h, int nrhs, const double* rr_stop);
int prcg_get_stops_rhs(prcg_t* h, int32_t* k_stop, int32_t* status);

/* ---- a BATCH of small independent systems, solved in one launch, one workgroup per system --------------------------------
 * Replaces the reference's loop over matrices and methods around `method(A, b, x0, max_iter, ...)` (numerical_experiments/
 * figure_gen.py:59, :245-339: the convergence table is small matrices times nine methods), and the loop a time stepper or a
 * parameter sweep runs over hundreds of right-hand sides of one small matrix.  n_sys systems A_s x_s = b_s; every one is solved
 * by the one-workgroup solver of a small single session (PRCG_SCHED_SMALL: the whole solve inside one launch of one 1024-thread
 * workgroup, matrix in registers or LDS), all of them in the SAME launch, the workgroup index selecting the system.  Systems
 * may differ in size and matrix; systems that share a matrix name the same one, which is uploaded once.
 *   prcg_batch_create  n_mat matrices concatenated: rows_off / nnz_off (n_mat + 1 int64 each, from 0); indptr int32, zero-based
 *                      PER MATRIX, n_m + 1 entries each (matrix m's start at rows_off[m] + m); indices int32 local columns
 *                      (matrix m's at nnz_off[m]); data likewise.  mat_of[s] in [0, n_mat): the matrix of system s.  A separate
 *                      object: it borrows the handle's device and compute stream, needs no operator on the handle and leaves one
 *                      there (and an open session) alone.  Destroy it before the handle.
 *   prcg_batch_begin   rhs, x0: the systems' vectors concatenated in system order.  variant: PRCG_PIPE_PR, PRCG_PIPE_PR_M or
 *                      PRCG_HS, unpreconditioned.  hist_mask: 0 or PRCG_HIST_UPDATED_RESIDUAL_2_NORM.  One launch per launch
 *                      group computes x = x0, r = b - A x0, p = r, s = A p and the initial inner products of every system.
 *                      May be called again: a new session on the same matrices.
 *   prcg_batch_begin_jacobi  the same three variants preconditioned by a diagonal scaling that is applied INSIDE the one-workgroup
 *                      solver: replaces the reference's `*_pcg` calls with the Jacobi lambda `(1/A.diagonal())*x` (figure_gen.py:43 and
 *                      the `*_pcg` half of the convergence table; pipe_pr_cg.py:109-193 for PRCG_PIPE_PR / PRCG_PIPE_PR_M, hs_cg.py:70-131
 *                      for PRCG_HS).  inv_diag: the systems' reciprocal diagonals concatenated in system order like rhs -- they belong
 *                      to the SYSTEM, not the matrix: two systems on one matrix may differ.  Its values are not inspected: a zero, inf
 *                      or nan poisons its own system only, as a bad right-hand side does.  One launch per group computes x = x0,
 *                      r = b - A x0, r~ = d r, p = r~, s = A p (pipelined: s~ = d s) and row 0 of the scalars.  The pipelined state is
 *                      the six vectors x, p, r, s, r~, s~ (w = A r~ and u = A s~ are formed anew in every iteration); scalars per
 *                      iteration {mu = p.s, delta = r.s~, gamma = s~.s, nu = r~.r, rr = r.r}, Hestenes-Stiefel {mu, -, -, nu, rr}; the
 *                      history is sqrt(rr).  The per-row expressions are those of a single Jacobi session: from the same state and
 *                      coefficients one iteration yields the same vectors, bit for bit.  The session then runs through
 *                      prcg_batch_iterate / _sync / the accessors below, unchanged.  With inv_diag = ones a system carries the bits of
 *                      prcg_batch_begin's.  Refused beside what prcg_batch_begin refuses: null inv_diag; a system whose matrix lives in
 *                      LDS and lies within 128 bytes of the cap -- the fifth inner product needs 128 bytes more (the text names the
 *                      first such system).
 *   prcg_batch_begin_block_jacobi  the same three variants preconditioned by POINT-BLOCK JACOBI applied inside the one-workgroup
 *                      solver: blocks that follow a partition of each system, every size in 1..8 (a uniform bs is the partition 0,
 *                      bs, 2 bs, ..., n with a short last block) -- prcg_set_block_jacobi_var for a batch.  nblk_off: n_sys + 1
 *                      int64 from 0, system s has nb_s = nblk_off[s+1] - nblk_off[s] blocks.  block_ptr: the partitions concatenated,
 *                      nb_s + 1 entries per system starting at nblk_off[s] + s, zero-based PER SYSTEM, first entry 0, last entry n_s
 *                      (the convention of indptr per matrix).  inv_blocks: the inverses of the diagonal blocks in the PACKED format
 *                      of prcg_set_block_jacobi_var -- block k as m_k x m_k doubles, row-major, no padding -- the systems
 *                      concatenated in system order.  Blocks belong to the SYSTEM, as inv_diag does: two systems on one matrix may
 *                      differ.  Values are not inspected: a nan poisons its own system only.  The apply is word for word the loop
 *                      of prcg_set_block_jacobi_var: row start + a of a block forms acc = B[a][0] * v[start], then acc = acc +
 *                      B[a][j] * v[start+j] for j ascending, every product and sum rounded, no FMA -- the bits of
 *                      VarBlockJacobi.__call__ and BlockJacobi.__call__ (cg_variants).  The rows of a block exchange v through LDS
 *                      inside the iteration; a block may lie anywhere in its system.  State, scalars, history and accessors are
 *                      those of prcg_batch_begin_jacobi: the pipelined state is x, p, r, s, r~, s~ (w = A r~ and u = A s~ formed
 *                      anew in every iteration), scalars {mu, delta, gamma, nu, rr}, Hestenes-Stiefel {mu, -, -, nu, rr};
 *                      PRCG_VEC_RT / _ST are readable in pipelined sessions; prcg_batch_iterate / _sync and the accessors serve
 *                      the session unchanged, and so does the stop (prcg_batch_set_stop / prcg_batch_get_stops).  Invariant: with
 *                      every block of size 1 and inv_blocks = d a system carries the bits of prcg_batch_begin_jacobi with inv_diag =
 *                      d (acc = B[0][0] * v is d * v).  Fit rule: that of prcg_batch_begin_jacobi, byte for byte -- matrix in registers:
 *                      always fits; matrix in LDS: 32 n + 640 + 12 nnz + 16 <= 159744 bytes.  The exchange adds no LDS: it uses the
 *                      buffer that otherwise takes the next iterate's pairs (the new r~, s~ overwrite the old in place), at the
 *                      price of one barrier more per iteration.  So n up to 4096 is served, four rows per thread.
 *                      Refused, each with PRCG_EINVAL and a text that names the reason and the first offending system, nothing
 *                      changed (an open session goes on): a null pointer; nblk_off not from 0 or decreasing; a partition whose
 *                      first entry is not 0 or whose last is not n_s; a block size outside 1..8 (system, block and size are
 *                      named); a variant, history bit or max_iter that the other begins refuse; a system that does not fit.
 *   prcg_batch_iterate enqueues; every system advances by iters (k + iters <= max_iter).  prcg_batch_sync waits.
 *   prcg_batch_set_stop  rr_stop: n_sys thresholds on r.r, one per system (for a tolerance tol on the 2-norm of the updated residual:
 *                      tol * tol), finite and >= 0; NULL clears them.  They are copied at the call -- the caller's buffer is theirs
 *                      again on return -- and apply to sessions BEGUN afterwards (prcg_batch_begin, prcg_batch_begin_jacobi and
 *                      prcg_batch_begin_block_jacobi, signatures unchanged); an open session is not affected.  In such a session every system stops by itself,
 *                      decided inside its workgroup without the host: after iteration k, and at k = 0 on the initial state, on row k
 *                      of its scalars, mu = [0], nu = [3], rr = [PRCG_S_RR], in this order:
 *                        1. rr <= rr_stop[s]                                   -> stop, status 1 (converged);
 *                        2. else !(0 < mu && mu < inf && 0 < nu && nu < inf)   -> stop, status 2 (breakdown: the next step's
 *                           alpha = nu / mu would not be that of an SPD system);
 *                        3. else go on (status 0, stop iteration -1).
 *                      A system stopped at k keeps the complete state of iteration k: x, r, p, s (and r~, s~) are those of
 *                      iteration k, scalar rows 0..k and coefficient rows 1..k are written, later rows stay at the zeros that begin
 *                      set, and later prcg_batch_iterate calls leave the system untouched -- its workgroup returns at once, which
 *                      makes room for the next one where the batch is larger than the chip.  A threshold of 0 stops on an exactly
 *                      zero residual (b = A x0) and on breakdown only.  A system that does not stop carries the bits of a session
 *                      without thresholds.  prcg_batch_iteration keeps counting what was launched, stopped systems or not.
 *                      Refused: a NaN, infinite or negative threshold (the text names the system; the thresholds set before stay).
 *   prcg_batch_get_stops  synchronises; k_stop[s], status[s] of the open session, n_sys int32 each: the iteration system s stopped
 *                      at and why (1 converged, 2 breakdown), or -1 and 0 while it runs -- and for every system of a session begun
 *                      without thresholds.  Refused without an open session.
 * Launch groups: the systems whose matrix lives in registers (n <= 1024, rows of at most 8) form one launch, those whose matrix
 * lives in LDS another; a call is one launch per group.
 * Bits: from the same state and scalars a system's iterations are those of a single small session on its matrix, bit for bit
 * -- vectors, inner products, coefficients, history -- whatever its position in the batch and whatever the other systems are; a
 * breakdown (inf / nan) of one system stays in that system.  The initial VECTORS carry the single session's bits too.  The
 * initial inner products (row 0 of the scalars) are summed in the workgroup's own order -- thread-sequential over rows tid,
 * tid + 1024, ..., wave butterfly, 16 waves: the order of the loop -- where the single session sums them in the order of its
 * start-up launches: row 0 may differ from a single session's in the last bit.
 * Refused (PRCG_EINVAL, the text names the reason and, for a reason that lies in one system, the first such system; nothing is
 * created or changed): create -- a null pointer, n_sys < 1, n_mat < 1, a communicator on the handle, inconsistent offsets
 * (rows_off / nnz_off not from 0 or a matrix without rows; an indptr that does not run from 0 to its matrix's nonzero count or
 * decreases), a column index outside its matrix, a mat_of entry out of range, a system that does not fit the one-workgroup
 * solver (a batch has no other schedule); begin -- another variant, another history bit, null rhs or x0, max_iter < 1.
 * Errors are reported through prcg_last_error of the handle the batch was created on.
 * Accessors (they synchronise): s = the system.  prcg_batch_get_vector: PRCG_VEC_X, _R, _P, _S, the system's n doubles, and in a
 * pipelined session begun with prcg_batch_begin_jacobi or prcg_batch_begin_block_jacobi also PRCG_VEC_RT, _ST (refused in any
 * other batch session);
 * prcg_batch_get_solutions: every x concatenated in system order, ONE copy; scalars / coefficients / history as
 * prcg_get_scalars / prcg_get_coefficients / prcg_get_history return them (history: max_iter doubles, nothing is written when
 * hist_mask was 0; entries up to min(k, the system's stop iteration), zeros beyond).  No setters, no recorder of state, no preconditioner but the diagonal scaling of prcg_batch_begin_jacobi and the
 * blocks of prcg_batch_begin_block_jacobi (no inverses built on the device, no callback). */
typedef struct prcg_batch prcg_batch_t;
int  prcg_batch_create(prcg_t* h, int n_mat, const int64_t* rows_off, const int64_t* nnz_off, const int32_t* indptr,
                       const int32_t* indices, const double* data, int n_sys, const int32_t* mat_of, prcg_batch_t** out);
void prcg_batch_destroy(prcg_batch_t* b);
int prcg_batch_begin(prcg_batch_t* b, int variant, const double* rhs, const double* x0, int max_iter, uint32_t hist_mask);
int prcg_batch_begin_jacobi(prcg_batch_t* b, int variant, const double* rhs, const double* x0, const double* inv_diag, int max_iter,
                            uint32_t hist_mask);
int prcg_batch_begin_block_jacobi(prcg_batch_t* b, int variant, const double* rhs, const double* x0, const int64_t* nblk_off,
                                  const int64_t* block_ptr, const double* inv_blocks, int max_iter, uint32_t hist_mask);
int prcg_batch_iterate(prcg_batch_t* b, int iters);
int prcg_batch_sync(prcg_batch_t* b);
int prcg_batch_iteration(const prcg_batch_t* b);
int prcg_batch_set_stop(prcg_batch_t* b, const double* rr_stop);
int prcg_batch_get_stops(prcg_batch_t* b, int32_t* k_stop, int32_t* status);
int prcg_batch_get_vector(prcg_batch_t* b, int which, int s, double* out);
int prcg_batch_get_solutions(prcg_batch_t* b, double* x_cat);
int prcg_batch_get_scalars(prcg_batch_t* b, int k, int s, double* out);
int prcg_batch_get_coefficients(prcg_batch_t* b, int k, int s, double* out);
int prcg_batch_get_history(prcg_batch_t* b, int s, double* hist);

/* HIP-event sampling of the SpMV/SpMM and update launches inside prcg_iterate:
 * every `stride`-th iteration is bracketed (0 = off).  Read back with prcg_get_timings. */
int prcg_set_profiling(prcg_t* h, int stride);
int prcg_get_timings(prcg_t* h, prcg_timings* t);

/* one call = begin + (max_iter-1) iterations + histories + x; the drop-in for
 * `method(A,b,x0,max_iter,...)`.  hist: [popcount(hist_mask)][max_iter], nullable. */
int prcg_solve(prcg_t* h, int variant, const double* b, const double* x0, int max_iter,
               const double* x_true, const double* inv_diag, uint32_t hist_mask,
               double* hist, double* x_out, prcg_timings* t);

#ifdef __cplusplus
}
#endif
#endif /* PRCG_H */
