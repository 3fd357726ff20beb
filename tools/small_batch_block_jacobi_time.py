"""B small systems solved as ONE block-Jacobi-preconditioned batch (device.DeviceBatch.begin(block_jacobi=...): one launch, one
workgroup per system, the blocks applied inside it) against
  (a) the same B systems under the existing JACOBI batch (inv_diag=...): per iteration, what the exchange between a block's
      rows -- one barrier and the LDS traffic of up to 8 pairs per row -- costs;
  (b) the same B systems solved one after another by single block-Jacobi sessions on an operator that is already uploaded --
      the stored-tilde schedule, several launches per iteration from the host: what a caller runs today;
  (c) `stops`: the nine test systems in one batch with rtol = 1e-8, blocks (bs 3) against Jacobi: mean stop iteration and the
      time of the batch.
   small_batch_block_jacobi_time.py [sizes=1,16,256,1024] [iters=1000] [repeats=5] [loop_iters=200]
Systems: nos7 (bs = 4) under pipe_pr_pcg and bcsstk03 (bs = 3) under hs_pcg (tests/golden fixtures), BlockJacobi's inverses,
right-hand sides b * (1 + s / B): distinct.  Method of small_batch_time.py: every leg is timed with the host clock around work
that ends in a synchronise, after one warm-up of each, `repeats` windows each, ALTERNATED in one process; the best and the
median are reported.  Two figures per leg: `solve` = begin + iterations, `iterate` = the iterations alone.  The iterations run to
`iters` whatever the residual does.  The loop of single sessions is timed on min(B, 16) systems and `loop_iters` iterations and
scaled to B systems and `iters` iterations (it is B independent sessions of equal cost, and one session's iterations cost the
same each): at B = 1024 and 1000 iterations it would take minutes.
One record per measurement on stderr, ONE JSON line on stdout."""
import json, sys, time
import numpy as np
from small_batch_timing import NINE, load_system, options, summary, timed, timed_loop
from new_cg_variants_amd import _lib as L
from new_cg_variants_amd.cg_variants import BlockJacobi, _batch_blocks
from new_cg_variants_amd.device import DeviceBatch, DeviceCSR

opt = options(dict(sizes='1,16,256,1024', iters='1000', repeats='5', loop_iters='200'), __doc__)
SIZES, ITERS, REPEATS, LOOP_ITERS = [int(q) for q in opt['sizes'].split(',')], int(opt['iters']), int(opt['repeats']), int(opt['loop_iters'])

result = {'iters': ITERS, 'cases': []}
for name, vname, bs in (('nos7', 'PIPE_PR', 4), ('bcsstk03', 'HS', 3)):
    A, b0 = load_system(name)
    n, variant = A.shape[0], getattr(L, vname)
    d = 1 / A.diagonal()
    prec = BlockJacobi(A, bs)
    pair = _batch_blocks('time', prec, [n])[0]
    op = DeviceCSR(A)
    op.begin(variant, b0, np.zeros(n), LOOP_ITERS + 1, hist_mask=1, block_jacobi=(bs, prec.inv_blocks))
    schedule = {k: v for k, v in op.schedule().items() if isinstance(v, (bool, int, str))}
    for nb in SIZES:
        B = np.array([b0 * (1 + s / nb) for s in range(nb)])
        X0 = np.zeros((nb, n))
        D = np.tile(d, (nb, 1))
        blocks = [pair] * nb
        nl = min(nb, 16)
        batch = DeviceBatch([A], np.zeros(nb, dtype=np.int32))
        timed(batch, variant, B, X0, ITERS, block_jacobi=blocks)         # warm-up of the three legs
        timed(batch, variant, B, X0, ITERS, inv_diag=D)
        timed_loop(op, variant, B[:min(nb, 4)], X0[:min(nb, 4)], LOOP_ITERS, block_jacobi=(bs, prec.inv_blocks))
        tb, tj, tl = [], [], []
        for r in range(REPEATS):
            tj.append(timed(batch, variant, B, X0, ITERS, inv_diag=D))
            tb.append(timed(batch, variant, B, X0, ITERS, block_jacobi=blocks))
            if r < 2:
                tl.append(timed_loop(op, variant, B[nb - nl:], X0[nb - nl:], LOOP_ITERS, block_jacobi=(bs, prec.inv_blocks)))
        # the batch and the loop computed the same thing: the last system's history, while two summation orders still agree
        timed(batch, variant, B, X0, 4, block_jacobi=blocks)
        hb = batch.history(nb - 1)['updated_residual_2_norm'][:5]
        timed(op, variant, B[nb - 1], X0[nb - 1], 4, block_jacobi=(bs, prec.inv_blocks))
        hl = op.history()['updated_residual_2_norm'][:5]
        dev = float(np.abs(hb / hl - 1).max())
        assert dev <= 1e-10, (hb, hl)
        batch.close()
        sb, sj, sl = summary(tb), summary(tj), summary(tl)
        loop_us = sl['iterate_ms_best'] * 1e3 / LOOP_ITERS / nl            # one single session, per iteration
        rec = {'matrix': name, 'n': n, 'variant': vname, 'bs': bs, 'B': nb, 'batch_blocks': sb, 'batch_jacobi': sj,
               'loop_blocks_measured': dict(sl, systems=nl, iters=LOOP_ITERS),
               'us_per_iteration_batch_blocks': sb['iterate_ms_best'] * 1e3 / ITERS,
               'us_per_iteration_batch_jacobi': sj['iterate_ms_best'] * 1e3 / ITERS,
               'us_per_iteration_single_blocks': loop_us,
               'loop_iterate_ms_scaled': loop_us * ITERS * nb / 1e3,
               'speedup_iterate_vs_loop': loop_us * ITERS * nb / 1e3 / sb['iterate_ms_best'],
               'cost_iterate_vs_jacobi': sb['iterate_ms_best'] / sj['iterate_ms_best'],
               'cost_solve_vs_jacobi': sb['solve_ms_best'] / sj['solve_ms_best'],
               'history_deviation_first5': dev, 'single_schedule': schedule}
        result['cases'].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    op.close()

# ---- the nine systems stopped at rtol = 1e-8: blocks (bs 3) against Jacobi, one batch each, alternated
systems = [load_system(name) for name in NINE]
mats, rhs = [A for A, _ in systems], [b for _, b in systems]
x0 = [np.zeros(b.size) for b in rhs]
thr = np.array([(1e-8 * np.linalg.norm(b)) ** 2 for b in rhs])
blocks = [_batch_blocks('time', BlockJacobi(A, 3), [A.shape[0]])[0] for A in mats]
diag = [1 / A.diagonal() for A in mats]
batch = DeviceBatch(mats)
MAXIT = 1000


def stopped(**begin):
    t0 = time.perf_counter()
    batch.begin(L.PIPE_PR, rhs, x0, MAXIT + 1, hist_mask=1, rr_stop=thr, **begin)
    batch.iterate(MAXIT)
    k_stop, status = batch.stops()
    return time.perf_counter() - t0, k_stop.tolist(), status.tolist()


stopped(block_jacobi=blocks), stopped(inv_diag=diag)
tb, tj = [], []
for r in range(REPEATS):
    tj.append(stopped(inv_diag=diag))
    tb.append(stopped(block_jacobi=blocks))
batch.close()
rec = {'systems': NINE, 'variant': 'PIPE_PR', 'rtol': 1e-8, 'max_iter': MAXIT, 'bs': 3,
       'blocks': {'k_stop': tb[0][1], 'status': tb[0][2], 'mean_k_stop': float(np.mean([k if s else MAXIT for k, s in zip(tb[0][1], tb[0][2])])),
                  'ms_best': min(t[0] for t in tb) * 1e3, 'ms_median': float(np.median([t[0] for t in tb])) * 1e3},
       'jacobi': {'k_stop': tj[0][1], 'status': tj[0][2], 'mean_k_stop': float(np.mean([k if s else MAXIT for k, s in zip(tj[0][1], tj[0][2])])),
                  'ms_best': min(t[0] for t in tj) * 1e3, 'ms_median': float(np.median([t[0] for t in tj])) * 1e3}}
result['stops'] = rec
print(json.dumps(rec), file=sys.stderr, flush=True)
print(json.dumps(result))
