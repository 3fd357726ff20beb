"""B small systems solved as ONE Jacobi-preconditioned batch (device.DeviceBatch.begin(inv_diag=...): one launch, one workgroup
per system, the scaling applied inside it) against
  (a) the same B systems solved one after another by single Jacobi sessions on an operator that is already uploaded -- the
      code a caller had before the preconditioned batch existed (a preconditioned single session does not take the
      one-workgroup route: one or more launches per iteration from the host);
  (b) the UNPRECONDITIONED batch of the same systems: what the extra state (r~, s~, d) and the fifth inner product cost.
   small_batch_jacobi_time.py [sizes=1,16,256,1024] [iters=1000] [repeats=5]
Systems: nos7 under pipe_pr_pcg and bcsstk03 under hs_pcg (tests/golden fixtures), d = 1 / diag(A), right-hand sides
b * (1 + s / B): distinct.  Method of small_batch_time.py: every leg is timed with the host clock around work that ends in a
synchronise, after one warm-up of each; `repeats` windows each (the loop: 2 from B = 256 on), alternated; the best and the
median are reported.  Two figures per leg: `solve` = begin + iterations, `iterate` = the iterations alone.  (The iterations run
to `iters` whatever the residual does: a system that has converged -- nos7 under Jacobi breaks down near k = 125 -- goes on
through the same instructions on inf / nan.)
One record per measurement on stderr, ONE JSON line on stdout."""
import json, sys
import numpy as np
from small_batch_timing import load_system, options, summary, timed, timed_loop
from new_cg_variants_amd import _lib as L
from new_cg_variants_amd.device import DeviceBatch, DeviceCSR

opt = options(dict(sizes='1,16,256,1024', iters='1000', repeats='5'), __doc__)
SIZES, ITERS, REPEATS = [int(q) for q in opt['sizes'].split(',')], int(opt['iters']), int(opt['repeats'])

result = {'iters': ITERS, 'cases': []}
for name, vname in (('nos7', 'PIPE_PR'), ('bcsstk03', 'HS')):
    A, b0 = load_system(name)
    n, variant = A.shape[0], getattr(L, vname)
    d = 1 / A.diagonal()
    op = DeviceCSR(A)
    op.begin(variant, b0, np.zeros(n), ITERS + 1, hist_mask=1, inv_diag=d)
    schedule = {k: v for k, v in op.schedule().items() if isinstance(v, (bool, int, str))}
    for nb in SIZES:
        B = np.array([b0 * (1 + s / nb) for s in range(nb)])
        X0 = np.zeros((nb, n))
        D = np.tile(d, (nb, 1))
        batch = DeviceBatch([A], np.zeros(nb, dtype=np.int32))
        timed(batch, variant, B, X0, ITERS, inv_diag=D)            # warm-up of the three legs
        timed(batch, variant, B, X0, ITERS)
        timed_loop(op, variant, B[:min(nb, 4)], X0[:min(nb, 4)], ITERS, inv_diag=d)
        reps_loop = REPEATS if nb < 256 else min(REPEATS, 2)
        tj, tu, tl = [], [], []
        for r in range(REPEATS):
            tu.append(timed(batch, variant, B, X0, ITERS))
            tj.append(timed(batch, variant, B, X0, ITERS, inv_diag=D))
            if r < reps_loop:
                tl.append(timed_loop(op, variant, B, X0, ITERS, inv_diag=d))
        # the batch and the loop computed the same thing: the last system's history, while two summation orders still agree
        hb = batch.history(nb - 1)['updated_residual_2_norm'][:5]
        hl = op.history()['updated_residual_2_norm'][:5]
        dev = float(np.abs(hb / hl - 1).max())
        assert dev <= 1e-10, (hb, hl)
        batch.close()
        sj, su, sl = summary(tj), summary(tu), summary(tl)
        rec = {'matrix': name, 'n': n, 'variant': vname, 'B': nb, 'batch_jacobi': sj, 'batch_unpreconditioned': su, 'loop_jacobi': sl,
               'us_per_iteration_batch_jacobi': sj['iterate_ms_best'] * 1e3 / ITERS,
               'us_per_iteration_batch_unpreconditioned': su['iterate_ms_best'] * 1e3 / ITERS,
               'us_per_iteration_single_jacobi': sl['iterate_ms_best'] * 1e3 / ITERS / nb,
               'speedup_solve_vs_loop': sl['solve_ms_best'] / sj['solve_ms_best'],
               'speedup_iterate_vs_loop': sl['iterate_ms_best'] / sj['iterate_ms_best'],
               'cost_iterate_vs_unpreconditioned': sj['iterate_ms_best'] / su['iterate_ms_best'],
               'cost_solve_vs_unpreconditioned': sj['solve_ms_best'] / su['solve_ms_best'],
               'history_deviation_first5': dev, 'single_schedule': schedule}
        result['cases'].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    op.close()
print(json.dumps(result))
