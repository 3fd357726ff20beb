"""B small systems solved as ONE batch (device.DeviceBatch: one launch, one workgroup per system) against the same B systems
solved one after another by single sessions on an operator that is already uploaded, in one process:
   small_batch_time.py [sizes=1,16,64,256,1024] [iters=1000] [repeats=5] [bins=1]
Systems: nos7 under pipe_pr_cg and bcsstk03 under hs_cg (tests/golden fixtures), right-hand sides b * (1 + s / B): distinct.
The single-session loop is the reference: DeviceCSR(A) once, then per system begin, iterate(iters), sync -- the code a caller
had before the batch existed.  Both legs are timed with the host clock around work that ends in a synchronise, after one
warm-up of each; `repeats` windows each (the loop: 3 from B = 256 on), alternated; the best and the median are reported.  Two
figures per leg: `solve` = begin + iterations (what a caller waits for), `iterate` = the iterations alone.
bins=1 also answers whether mode-0 launches should be split by LDS size: 512 systems of model_48_8_3 (30 KB of LDS each) alone,
and the same 512 beside ONE laplace_2d(40, 40) whose 145,808 B every workgroup of the launch then reserves.
One record per measurement on stderr, ONE JSON line on stdout."""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import scipy.sparse as sp
from new_cg_variants_amd import problems as P, _lib as L
from new_cg_variants_amd.device import DeviceBatch, DeviceCSR



def load_matrix(name):
    z = np.load(os.path.join(ROOT, 'tests', 'golden', f'matrix_{name}.npz'))
    n = int(z['n'])
    return sp.csr_matrix((z['data'], z['indices'], z['indptr']), shape=(n, n)), z


opt = dict(sizes='1,16,64,256,1024', iters='1000', repeats='5', bins='1')
for a in sys.argv[1:]:
    k, _, v = a.partition('=')
    if k not in opt or not v:
        sys.exit(f'unknown argument {a!r}\n{__doc__}')
    opt[k] = v
SIZES, ITERS, REPEATS = [int(q) for q in opt['sizes'].split(',')], int(opt['iters']), int(opt['repeats'])


def timed_batch(batch, variant, B, X0):
    t0 = time.perf_counter()
    batch.begin(variant, B, X0, ITERS + 1, hist_mask=1)
    t1 = time.perf_counter()
    batch.iterate(ITERS)
    batch.sync()
    t2 = time.perf_counter()
    return t2 - t0, t2 - t1


def timed_loop(op, variant, B, X0):
    solve = it = 0.0
    for b, x0 in zip(B, X0):
        t0 = time.perf_counter()
        op.begin(variant, b, x0, ITERS + 1, hist_mask=1)
        t1 = time.perf_counter()
        op.iterate(ITERS)
        op.sync()
        t2 = time.perf_counter()
        solve += t2 - t0
        it += t2 - t1
    return solve, it


def summary(samples):
    a = np.array(samples) * 1e3
    return {'solve_ms_best': float(a[:, 0].min()), 'solve_ms_median': float(np.median(a[:, 0])),
            'iterate_ms_best': float(a[:, 1].min()), 'iterate_ms_median': float(np.median(a[:, 1]))}


result = {'iters': ITERS, 'cases': []}
for name, vname in (('nos7', 'PIPE_PR'), ('bcsstk03', 'HS')):
    A, z = load_matrix(name)
    n, variant = A.shape[0], getattr(L, vname)
    b0 = np.asarray(z['b'], dtype=np.float64)
    op = DeviceCSR(A)
    op.begin(variant, b0, np.zeros(n), ITERS + 1, hist_mask=1)
    assert op.schedule()['small']
    for nb in SIZES:
        B = np.array([b0 * (1 + s / nb) for s in range(nb)])
        X0 = np.zeros((nb, n))
        batch = DeviceBatch([A], np.zeros(nb, dtype=np.int32))
        timed_batch(batch, variant, B, X0)            # warm-up of both legs
        timed_loop(op, variant, B[:min(nb, 4)], X0[:min(nb, 4)])
        reps_loop = REPEATS if nb < 256 else min(REPEATS, 3)
        tb, tl = [], []
        for r in range(REPEATS):
            tb.append(timed_batch(batch, variant, B, X0))
            if r < reps_loop:
                tl.append(timed_loop(op, variant, B, X0))
        # the two legs computed the same thing: the last system's history, to the bar between two summation orders of row 0
        hb = batch.history(nb - 1)['updated_residual_2_norm'][:8]
        hl = op.history()['updated_residual_2_norm'][:8]
        assert np.allclose(hb, hl, rtol=1e-12, atol=0), (hb, hl)
        batch.close()
        sb, sl = summary(tb), summary(tl)
        rec = {'matrix': name, 'n': n, 'variant': vname, 'B': nb, 'batch': sb, 'loop': sl,
               'us_per_iteration_batch': sb['iterate_ms_best'] * 1e3 / ITERS,
               'us_per_iteration_single': sl['iterate_ms_best'] * 1e3 / ITERS / nb,
               'speedup_solve': sl['solve_ms_best'] / sb['solve_ms_best'], 'speedup_iterate': sl['iterate_ms_best'] / sb['iterate_ms_best']}
        result['cases'].append(rec)
        print(json.dumps(rec), file=sys.stderr, flush=True)
    op.close()

if int(opt['bins']):
    A48 = load_matrix('model_48_8_3')[0]
    big = P.laplace_2d(40, 40)
    nb = 512
    B48 = [np.ones(48) * (1 + s / nb) for s in range(nb)]
    legs = {'alone': DeviceBatch([A48], np.zeros(nb, dtype=np.int32)),
            'beside_145KB': DeviceBatch([A48, big], np.array([0] * nb + [1], dtype=np.int32))}
    args = {'alone': (B48, [np.zeros(48)] * nb), 'beside_145KB': (B48 + [np.ones(1600)], [np.zeros(48)] * nb + [np.zeros(1600)])}
    # (the big member alone, so that its own time can be told from what it costs the others)
    legs['big_alone'] = DeviceBatch([big])
    args['big_alone'] = ([np.ones(1600)], [np.zeros(1600)])
    times = {k: [] for k in legs}
    for r in range(REPEATS + 1):
        for k, batch in legs.items():
            t = timed_batch(batch, L.PIPE_PR, *args[k])
            if r:
                times[k].append(t)
    result['mode0_bins'] = {k: summary(v) for k, v in times.items()}
    print(json.dumps(result['mode0_bins']), file=sys.stderr, flush=True)
    for batch in legs.values():
        batch.close()
print(json.dumps(result))
