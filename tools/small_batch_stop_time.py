"""What the per-system stop of a batch (device.DeviceBatch.begin(rr_stop=...): every system stops at its own threshold on r.r,
decided inside its workgroup) costs and what it saves.
  (a) the CHECK: B systems on one matrix, `iters` iterations, the scaling d = ones (the preconditioned bodies, Jacobi off) and
      rr_stop = 0, so that nothing stops, against the same object begun WITHOUT thresholds -- the kernels as they were before
      the stop existed.  nos7 under pipe_pr_pcg and bcsstk03 under hs_pcg.  (`stopped` counts the systems that stopped all the
      same -- on a breakdown; the ratio means what it says only where it is 0.)
  (b) the SAVING: the nine test systems of tests/test_small_batch.py under Jacobi, repeated to B systems (system s uses matrix
      s mod 9), pipe_pr_pcg, `mix_iters` iterations, with rtol = 1e-8 against without.  `mean_stop` is the mean over the systems
      of the iteration they stopped at (mix_iters for one that ran out), `max_stop` the largest: whether the time follows the
      one or the other is the thing to read off.
   small_batch_stop_time.py [sizes=1,16,256,1024] [iters=1000] [mix_iters=150] [repeats=5]
Method of small_batch_time.py: every leg is timed with the host clock around work that ends in a synchronise, after one warm-up
of each; `repeats` windows each, alternated; the best and the median are reported.  Two figures per leg: `solve` = begin +
iterations, `iterate` = the iterations alone.  One process.
One record per measurement on stderr, ONE JSON line on stdout."""
import json, sys
import numpy as np
from small_batch_timing import NINE, load_system, options, summary, timed
from new_cg_variants_amd import _lib as L
from new_cg_variants_amd.device import DeviceBatch

opt = options(dict(sizes='1,16,256,1024', iters='1000', mix_iters='150', repeats='5'), __doc__)
SIZES, ITERS, MIX_ITERS, REPEATS = [int(q) for q in opt['sizes'].split(',')], int(opt['iters']), int(opt['mix_iters']), int(opt['repeats'])


def compare(batch, variant, B, X0, D, iters, rr_stop):
    """windows of the session with thresholds and without, alternated after a warm-up of each; the stop words of the last one with"""
    timed(batch, variant, B, X0, iters, inv_diag=D, rr_stop=rr_stop)
    timed(batch, variant, B, X0, iters, inv_diag=D)
    ts, tp = [], []
    for _ in range(REPEATS):
        tp.append(timed(batch, variant, B, X0, iters, inv_diag=D))
        ts.append(timed(batch, variant, B, X0, iters, inv_diag=D, rr_stop=rr_stop))
    k_stop, status = batch.stops()
    return summary(ts), summary(tp), k_stop, status


result = {'iters': ITERS, 'mix_iters': MIX_ITERS, 'check': [], 'saving': []}
# ---- (a) what the check costs ----
for name, vname in (('nos7', 'PIPE_PR'), ('bcsstk03', 'HS')):
    A, b0 = load_system(name)
    n, variant = A.shape[0], getattr(L, vname)
    for nb in SIZES:
        B = np.array([b0 * (1 + s / nb) for s in range(nb)])
        X0, D = np.zeros((nb, n)), np.ones((nb, n))
        batch = DeviceBatch([A], np.zeros(nb, dtype=np.int32))
        ss, sp_, k_stop, status = compare(batch, variant, B, X0, D, ITERS, 0.0)
        batch.close()
        rec = {'matrix': name, 'n': n, 'variant': vname, 'B': nb, 'with_check': ss, 'without': sp_, 'stopped': int(np.count_nonzero(status)),
               'us_per_iteration_with_check': ss['iterate_ms_best'] * 1e3 / ITERS, 'us_per_iteration_without': sp_['iterate_ms_best'] * 1e3 / ITERS,
               'cost_iterate_best': ss['iterate_ms_best'] / sp_['iterate_ms_best'],
               'cost_iterate_median': ss['iterate_ms_median'] / sp_['iterate_ms_median']}
        result['check'].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
# ---- (b) what stopping saves ----
systems = [load_system(name) for name in NINE]
for nb in SIZES:
    of = [s % 9 for s in range(nb)]
    B = [systems[m][1] for m in of]
    X0 = [np.zeros(b.size) for b in B]
    D = [1 / systems[m][0].diagonal() for m in of]
    thr = np.array([(1e-8 * np.linalg.norm(b)) ** 2 for b in B])
    batch = DeviceBatch([A for A, _ in systems[:min(nb, 9)]], np.array(of, dtype=np.int32))
    ss, sp_, k_stop, status = compare(batch, L.PIPE_PR, B, X0, D, MIX_ITERS, thr)
    batch.close()
    work = np.where(status != 0, k_stop, MIX_ITERS)
    rec = {'B': nb, 'variant': 'PIPE_PR', 'with_stop': ss, 'without': sp_, 'converged': int(np.count_nonzero(status == 1)),
           'breakdown': int(np.count_nonzero(status == 2)), 'ran_out': int(np.count_nonzero(status == 0)),
           'mean_stop': float(work.mean()), 'max_stop': int(work.max()),
           'time_iterate_best_vs_without': ss['iterate_ms_best'] / sp_['iterate_ms_best'],
           'time_iterate_median_vs_without': ss['iterate_ms_median'] / sp_['iterate_ms_median'],
           'time_solve_best_vs_without': ss['solve_ms_best'] / sp_['solve_ms_best']}
    result['saving'].append(rec)
    print(json.dumps(rec), file=sys.stderr, flush=True)
print(json.dumps(result))
