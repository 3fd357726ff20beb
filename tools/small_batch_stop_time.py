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
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import scipy.sparse as sp
from new_cg_variants_amd import _lib as L
from new_cg_variants_amd import problems
from new_cg_variants_amd.device import DeviceBatch

NINE = ['bcsstk03', 'nos4', 'bcsstm22', 'nos7', 'lap32x32', '494_bus', 'model_48_8_3', 'lap40x40', 'lap33x32']


def load_system(name):
    if name.startswith('lap'):
        nx, ny = (int(q) for q in name[3:].split('x'))
        A = problems.laplace_2d(nx, ny)
        return A, np.ones(A.shape[0])
    z = np.load(os.path.join(ROOT, 'tests', 'golden', f'matrix_{name}.npz'))
    n = int(z['n'])
    return sp.csr_matrix((z['data'], z['indices'], z['indptr']), shape=(n, n)), np.asarray(z['b'], dtype=np.float64)


opt = dict(sizes='1,16,256,1024', iters='1000', mix_iters='150', repeats='5')
for a in sys.argv[1:]:
    k, _, v = a.partition('=')
    if k not in opt or not v:
        sys.exit(f'unknown argument {a!r}\n{__doc__}')
    opt[k] = v
SIZES, ITERS, MIX_ITERS, REPEATS = [int(q) for q in opt['sizes'].split(',')], int(opt['iters']), int(opt['mix_iters']), int(opt['repeats'])


def timed(batch, variant, B, X0, D, iters, rr_stop):
    t0 = time.perf_counter()
    batch.begin(variant, B, X0, iters + 1, hist_mask=1, inv_diag=D, rr_stop=rr_stop)
    t1 = time.perf_counter()
    batch.iterate(iters)
    batch.sync()
    t2 = time.perf_counter()
    return t2 - t0, t2 - t1


def summary(samples):
    a = np.array(samples) * 1e3
    return {'solve_ms_best': float(a[:, 0].min()), 'solve_ms_median': float(np.median(a[:, 0])),
            'iterate_ms_best': float(a[:, 1].min()), 'iterate_ms_median': float(np.median(a[:, 1]))}


def compare(batch, variant, B, X0, D, iters, rr_stop):
    """windows of the session with thresholds and without, alternated after a warm-up of each; the stop words of the last one with"""
    timed(batch, variant, B, X0, D, iters, rr_stop)
    timed(batch, variant, B, X0, D, iters, None)
    ts, tp = [], []
    for _ in range(REPEATS):
        tp.append(timed(batch, variant, B, X0, D, iters, None))
        ts.append(timed(batch, variant, B, X0, D, iters, rr_stop))
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
