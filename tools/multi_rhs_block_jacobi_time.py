"""Time of one block-Jacobi-preconditioned iteration of TWO right-hand sides, three ways, on one operator in one process:
   multi_rhs_block_jacobi_time.py [workload=s4b_80] [variant=hs] [bs=3] [legs=abc] [repeats=3] [window=0.5] [ceiling=1]
     a  the two-RHS block-Jacobi session (prcg_solve_begin_multi_block_jacobi: one two-vector product and one pass over the
        blocks per iteration serve both systems; the inner products that need M^-1 come out of the launch that applies it)
     b  two single block-Jacobi sessions of the same variant (hs_pcg; variant=pr: pr_pcg, m: m_pcg) on the same handle, one
        after the other -- what there was before.  legs=b uses nothing the new session added, so this file also runs against
        an older build of the package (copied into that tree's tools/)
     c  the two-RHS session with Jacobi (prcg_solve_begin_multi with inv_diag), for context
The blocks are built on the device from the operator (build_block_jacobi(bs)) once per handle and stay in force.
The legs are alternated, `repeats` times each.  A window is `iterate(K)` + `sync` under the host clock after a warm-up, K chosen
so that it lasts at least `window` seconds; leg b's window is the sum of its two sessions' windows of K iterations each (session
set-up is outside the clock in every leg).  The figure is microseconds per iteration OF BOTH SYSTEMS.
One record per window on stderr; ONE JSON line on stdout: per leg the median, min and max of the repeats, the ratio b / a of the
medians, and whether a is faster than b by more than the spread of the repeats of both legs.
ceiling=1 adds what prcg_stream_ceiling (mode 1) reaches in this process, the yardstick for the block launches: under
`rocprofv3 --kernel-trace --stats -- python tools/multi_rhs_block_jacobi_time.py legs=a repeats=1` k_block_jacobi_dots moves
(bs + 4) * 8 n useful bytes per launch in mode NU (Hestenes-Stiefel) and (bs + 8) * 8 n in mode PR (variant=pr, m)."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401
from new_cg_variants_amd import problems as P, _lib as L
from new_cg_variants_amd.device import DeviceCSR

opt = dict(workload='s4b_80', variant='hs', bs='3', legs='abc', repeats='3', window='0.5', ceiling='1')
for a in sys.argv[1:]:
    k, _, v = a.partition('=')
    if k not in opt or not v:
        sys.exit(f'unknown argument {a!r}\n{__doc__}')
    opt[k] = v
if set(opt['legs']) - set('abc') or opt['variant'] not in ('hs', 'pr', 'm') or not 1 <= int(opt['bs']) <= 8:
    sys.exit(__doc__)
repeats, window, bs = int(opt['repeats']), float(opt['window']), int(opt['bs'])
MAX_ITER, WARM, CALIB = 6000, 5, 5
VARIANT = {'hs': L.HS, 'pr': L.PR, 'm': L.M}[opt['variant']]

t0 = time.perf_counter()
wl = P.WORKLOADS[opt['workload']]
A = wl['make']()
n, nnz = A.shape[0], int(A.nnz)
B = np.stack([P.reference_rhs(A, n)[0], np.random.default_rng(7).standard_normal(n)])
X0 = np.zeros((2, n))
d = 1 / A.diagonal()
print(f'# {wl["desc"]}: n = {n} nnz = {nnz}, generated in {time.perf_counter() - t0:.1f} s', file=sys.stderr, flush=True)
op = DeviceCSR(A)
BLOCKS = dict(block_jacobi=(bs, None))          # built on the device; begin() rebuilds only if they are not in force


def timed(k):
    t = time.perf_counter()
    op.iterate(k)
    op.sync()
    return time.perf_counter() - t


def window_of(begin, target, k_fixed=None):
    """warm-up, calibration, one window of K iterations (at least `target` seconds) of the session `begin` opens: (K, seconds)"""
    begin()
    timed(WARM)
    per = timed(CALIB) / CALIB
    k = k_fixed or int(min(MAX_ITER - WARM - CALIB - 2, max(CALIB, np.ceil(1.15 * target / per))))
    return k, timed(k)


def finite_nu(columns):
    return all(bool(np.isfinite(op.get_scalars(op.k, rhs=j)[L.S_NU])) for j in range(columns))


result = {'workload': opt['workload'], 'variant': opt['variant'], 'bs': bs, 'n': n, 'nnz': nnz, 'operator_bytes': op.operator_bytes(),
          'window_s': window, 'repeats': repeats}
us = {leg: [] for leg in opt['legs']}
for rep in range(repeats):
    for leg in opt['legs']:
        if leg == 'a':
            k, dt = window_of(lambda: op.begin_multi_block_jacobi(VARIANT, B, X0, MAX_ITER, **BLOCKS), window)
            finite = finite_nu(2)
        elif leg == 'c':
            op.clear_preconditioners()
            k, dt = window_of(lambda: op.begin_multi(VARIANT, B, X0, MAX_ITER, inv_diag=d), window)
            finite = finite_nu(2)
        else:
            # each session half a window: the pair of sessions is one window of K iterations of both systems
            k, dt0 = window_of(lambda: op.begin(VARIANT, B[0], X0[0], MAX_ITER, **BLOCKS), window / 2)
            finite = bool(np.isfinite(op.get_scalars(op.k)[L.S_NU]))
            _, dt1 = window_of(lambda: op.begin(VARIANT, B[1], X0[1], MAX_ITER, **BLOCKS), window / 2, k)
            finite = finite and bool(np.isfinite(op.get_scalars(op.k)[L.S_NU]))
            dt = dt0 + dt1
        s = op.schedule()
        rec = {'workload': opt['workload'], 'variant': opt['variant'], 'leg': leg, 'repeat': rep, 'iterations': k, 'seconds': dt,
               'us_per_iteration_of_both': dt / k * 1e6, 'rhs2': s.get('rhs2', False), 'block_jacobi': s['block_jacobi'],
               'fused': s['fused'], 'sliced_rows': s['sliced_rows'], 'window': s['window'], 'finite': finite}
        print('# ' + json.dumps(rec), file=sys.stderr, flush=True)
        us[leg].append(rec['us_per_iteration_of_both'])
out = {leg: {'median_us': float(np.median(v)), 'min_us': min(v), 'max_us': max(v)} for leg, v in us.items()}
if 'a' in us and 'b' in us:
    out['ratio_b_over_a'] = out['b']['median_us'] / out['a']['median_us']
    spread = (out['a']['max_us'] - out['a']['min_us']) + (out['b']['max_us'] - out['b']['min_us'])
    out['a_faster_by_more_than_the_spread'] = bool(out['b']['median_us'] - out['a']['median_us'] > spread)
result['legs'] = out
if opt['ceiling'] == '1':
    result['stream_ceiling_mode1_gbs'] = op.stream_ceiling(max(n, 1 << 20) * 4, 1)
op.close()
print(json.dumps(result), flush=True)
