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
import json, sys
import numpy as np
from small_batch_timing import load_system, options, summary, timed, timed_loop
from new_cg_variants_amd import problems as P, _lib as L
from new_cg_variants_amd.device import DeviceBatch, DeviceCSR

opt = options(dict(sizes='1,16,64,256,1024', iters='1000', repeats='5', bins='1'), __doc__)
SIZES, ITERS, REPEATS = [int(q) for q in opt['sizes'].split(',')], int(opt['iters']), int(opt['repeats'])

result = {'iters': ITERS, 'cases': []}
for name, vname in (('nos7', 'PIPE_PR'), ('bcsstk03', 'HS')):
    A, b0 = load_system(name)
    n, variant = A.shape[0], getattr(L, vname)
    op = DeviceCSR(A)
    op.begin(variant, b0, np.zeros(n), ITERS + 1, hist_mask=1)
    assert op.schedule()['small']
    for nb in SIZES:
        B = np.array([b0 * (1 + s / nb) for s in range(nb)])
        X0 = np.zeros((nb, n))
        batch = DeviceBatch([A], np.zeros(nb, dtype=np.int32))
        timed(batch, variant, B, X0, ITERS)            # warm-up of both legs
        timed_loop(op, variant, B[:min(nb, 4)], X0[:min(nb, 4)], ITERS)
        reps_loop = REPEATS if nb < 256 else min(REPEATS, 3)
        tb, tl = [], []
        for r in range(REPEATS):
            tb.append(timed(batch, variant, B, X0, ITERS))
            if r < reps_loop:
                tl.append(timed_loop(op, variant, B, X0, ITERS))
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
    A48 = load_system('model_48_8_3')[0]
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
            t = timed(batch, L.PIPE_PR, *args[k], ITERS)
            if r:
                times[k].append(t)
    result['mode0_bins'] = {k: summary(v) for k, v in times.items()}
    print(json.dumps(result['mode0_bins']), file=sys.stderr, flush=True)
    for batch in legs.values():
        batch.close()
print(json.dumps(result))
