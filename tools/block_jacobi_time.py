"""Time per iteration of a block-Jacobi preconditioned solve, three ways, on one operator in one process:
   block_jacobi_time.py [workload=s4b_80] [bs=3] [variants=hs_pcg,pipe_pr_pcg] [legs=abc] [repeats=3] [window=0.5] [ceiling=1]
     a  device block Jacobi (prcg_set_block_jacobi: one kernel launch per application)
     b  the same BlockJacobi object through the host callback (prcg_set_preconditioner: two copies over the host link and a
        stream synchronisation per application) -- the only way to run it without the device path
     c  device Jacobi (inv_diag), for context: the one-launch schedules
The legs are alternated, `repeats` times each; a window is `iterate(K)` + `sync` under the host clock with K chosen so that it
lasts at least `window` seconds, after a warm-up.  One JSON line per window, then a markdown table (median, min..max).
ceiling=1 also prints what prcg_stream_ceiling (mode 1) reaches in this process, the yardstick for the kernel's own time:
under `rocprofv3 --kernel-trace --stats -- python tools/block_jacobi_time.py legs=a` the single-vector kernel moves
(bs + 2) * 8 * n bytes per launch and the pair kernel (bs + 4) * 8 * n."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401
from new_cg_variants_amd import problems as P, _lib as L
from new_cg_variants_amd.cg_variants import BlockJacobi
from new_cg_variants_amd.device import DeviceCSR

opt = dict(workload='s4b_80', bs='3', variants='hs_pcg,pipe_pr_pcg', legs='abc', repeats='3', window='0.5', ceiling='1')
for a in sys.argv[1:]:
    k, _, v = a.partition('=')
    if k not in opt or not v:
        sys.exit(f'unknown argument {a!r}\n{__doc__}')
    opt[k] = v
bs, repeats, window = int(opt['bs']), int(opt['repeats']), float(opt['window'])
VARIANT = {'hs_pcg': L.HS, 'pipe_pr_pcg': L.PIPE_PR, 'pipe_p_pcg': L.PIPE_P, 'pr_pcg': L.PR, 'cg_pcg': L.CG_CG, 'gv_pcg': L.GV}
MAX_ITER, WARM, CALIB = 6000, 5, 5

t0 = time.perf_counter()
wl = P.WORKLOADS[opt['workload']]
A = wl['make']()
n, nnz = A.shape[0], int(A.nnz)
b, x0, _ = P.reference_rhs(A, n)
print(f'# {wl["desc"]}: n = {n} nnz = {nnz}, generated in {time.perf_counter() - t0:.1f} s', file=sys.stderr, flush=True)
t0 = time.perf_counter()
prec = BlockJacobi(A, bs)
inv_diag = 1 / A.diagonal()
print(f'# {n // bs} diagonal blocks of size {bs} gathered and inverted in {time.perf_counter() - t0:.1f} s', file=sys.stderr, flush=True)
op = DeviceCSR(A)


def begin(leg, variant):
    if leg == 'a':
        op.begin(variant, b, x0, MAX_ITER, block_jacobi=(prec.bs, prec.inv_blocks))
    elif leg == 'b':
        op.begin(variant, b, x0, MAX_ITER, preconditioner=lambda v: prec(v))
    else:
        op.begin(variant, b, x0, MAX_ITER, inv_diag=inv_diag)


def timed(k):
    t = time.perf_counter()
    op.iterate(k)
    op.sync()
    return time.perf_counter() - t


rows = {}
for name in opt['variants'].split(','):
    variant = VARIANT[name]
    for rep in range(repeats):
        for leg in opt['legs']:
            begin(leg, variant)
            timed(WARM)
            per = timed(CALIB) / CALIB
            k = int(min(MAX_ITER - WARM - CALIB - 2, max(CALIB, np.ceil(window / per))))
            dt = timed(k)
            s = op.schedule()
            rec = {'workload': opt['workload'], 'n': n, 'bs': bs, 'variant': name, 'leg': leg, 'repeat': rep, 'iterations': k, 'seconds': dt,
                   'us_per_iteration': dt / k * 1e6, 'block_jacobi': s['block_jacobi'], 'fused': s['fused'], 'sliced_rows': s['sliced_rows'],
                   'finite': bool(np.isfinite(op.get_scalars(WARM + CALIB + k)[L.S_NU]))}
            print(json.dumps(rec), flush=True)
            rows.setdefault((name, leg), []).append(rec['us_per_iteration'])
if opt['ceiling'] == '1':
    gbs = op.stream_ceiling(max(n, 1 << 20) * 4, 1)
    print(json.dumps({'stream_ceiling_mode1': gbs}), flush=True)
op.close()

LEG = {'a': 'device block Jacobi', 'b': 'host callback, same object', 'c': 'device Jacobi'}
print(f'\n| {opt["workload"]} (n = {n}), bs = {bs} | leg | us / iteration: median (min .. max of {repeats}) |\n|---|---|---|')
for (name, leg), v in rows.items():
    print(f'| {name} | ({leg}) {LEG[leg]} | {np.median(v):.1f} ({min(v):.1f} .. {max(v):.1f}) |')
