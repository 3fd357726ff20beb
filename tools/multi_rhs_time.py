"""Time of one Hestenes-Stiefel (variant=pr, m: predict-and-recompute) iteration of TWO right-hand sides, two ways, on one
operator in one process:
   multi_rhs_time.py [workload=s4b_80] [variant=hs] [prec=none] [legs=ab] [repeats=3] [window=0.5] [ceiling=1]
     a  the two-RHS session (prcg_solve_begin_multi: one two-vector product per iteration serves both systems)
     b  two single hs_cg (prec=jacobi: hs_pcg) sessions on the same handle, one after the other -- what there was before;
        variant=pr: pr_cg / pr_pcg, variant=m: m_cg / m_pcg
   prec: none | jacobi | none,jacobi (both, one after the other, in this process).
The legs are alternated, `repeats` times each.  A window is `iterate(K)` + `sync` under the host clock after a warm-up, K
chosen so that it lasts at least `window` seconds; leg b's window is the sum of its two sessions' windows of K iterations
each (session set-up is outside the clock in both legs).  The figure is microseconds per iteration OF BOTH SYSTEMS.
One record per window on stderr; ONE JSON line on stdout: per prec and leg the median, min and max of the repeats, the ratio
b / a of the medians, and whether a exceeds b by more than the spread of the repeats of both legs.
ceiling=1 adds what prcg_stream_ceiling (mode 1) reaches in this process, the yardstick for the vector kernels: under
`rocprofv3 --kernel-trace --stats -- python tools/multi_rhs_time.py legs=a repeats=1` k_hs2_update_xr moves 96 n bytes per
launch (120 n with Jacobi), k_hs2_update_p 48 n, k_hs2_dot_ps 32 n; variant=pr: k_pr2_update 112 n (160 n), k_pr2_dots 48 n (72 n).
legs=b uses nothing the two-RHS session added, so this file also runs against an older build of the package.

nrhs=4: FOUR right-hand sides, three legs, the figure is microseconds per iteration OF ALL FOUR SYSTEMS:
     a  the four-RHS session (one four-vector product per iteration on sliced-row operators)
     b  two two-RHS sessions of K iterations each on the same handle, one after the other -- what there was before
     c  the four-RHS session on a second handle with PRCG_SPMM4=0 (two two-vector launches): c against a isolates the kernel
   `knobs=PRCG_SELL_WINDOW:0,...` sets switches on every handle (delta codes instead of window codes, for instance).
   With nrhs=4, legs=b uses nothing the four-RHS session added and runs against a build without it.

variant=pipe_pr | pipe_pr_m (nrhs=2): the PIPELINED predict-and-recompute iteration, three legs, microseconds per iteration OF BOTH SYSTEMS:
     a  the pipelined two-RHS session (prcg_solve_begin_multi_pipe: one update launch and ONE product of four vectors per iteration)
     b  two single default sessions of pipe_pr_cg (prec=jacobi: pipe_pr_pcg; pipe_pr_m: pipe_pr_m_cg / pipe_pr_m_pcg) on the same
        handle, one after the other, each ONE launch per iteration -- what there was before; runs against a build without the session
     c  the pipelined two-RHS session on a second handle with PRCG_SPMM4=0 (two two-vector launches): c against a isolates the
        four-vector kernel (profiles/multi_rhs_pipe.md)"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: F401
from new_cg_variants_amd import problems as P, _lib as L
from new_cg_variants_amd.device import DeviceCSR

opt = dict(workload='s4b_80', variant='hs', prec='none', legs='ab', repeats='3', window='0.5', ceiling='1', nrhs='2', knobs='')
for a in sys.argv[1:]:
    k, _, v = a.partition('=')
    if k not in opt or not v:
        sys.exit(f'unknown argument {a!r}\n{__doc__}')
    opt[k] = v
repeats, window = int(opt['repeats']), float(opt['window'])
if opt['nrhs'] not in ('2', '4') or set(opt['legs']) - set('ab' if opt['nrhs'] == '2' and not opt['variant'].startswith('pipe') else 'abc') or set(opt['prec'].split(',')) - {'none', 'jacobi'} or opt['variant'] not in ('hs', 'pr', 'm', 'pipe_pr', 'pipe_pr_m'):
    sys.exit(__doc__)
PIPE = opt['variant'].startswith('pipe')
if PIPE and opt['nrhs'] != '2':
    sys.exit('variant=pipe_pr / pipe_pr_m: nrhs=2 only\n' + __doc__)
MAX_ITER, WARM, CALIB = 6000, 5, 5
VARIANT = {'hs': L.HS, 'pr': L.PR, 'm': L.M, 'pipe_pr': L.PIPE_PR, 'pipe_pr_m': L.PIPE_PR_M}[opt['variant']]
NRHS = int(opt['nrhs'])
KNOBS = dict(kv.split(':', 1) for kv in opt['knobs'].split(',') if kv)

t0 = time.perf_counter()
wl = P.WORKLOADS[opt['workload']]
A = wl['make']()
n, nnz = A.shape[0], int(A.nnz)
B = np.stack([P.reference_rhs(A, n)[0]] + [np.random.default_rng(7 + j).standard_normal(n) for j in range(NRHS - 1)])
X0 = np.zeros((NRHS, n))
print(f'# {wl["desc"]}: n = {n} nnz = {nnz}, generated in {time.perf_counter() - t0:.1f} s', file=sys.stderr, flush=True)
op = DeviceCSR(A, knobs=KNOBS or None)
op_c = DeviceCSR(A, knobs=dict(KNOBS, PRCG_SPMM4='0')) if 'c' in opt['legs'] else None      # leg c: the product as two launches


def timed(k, o=None):
    o = o or op
    t = time.perf_counter()
    o.iterate(k)
    o.sync()
    return time.perf_counter() - t


def window_of(begin, target, k_fixed=None, o=None):
    """warm-up, calibration, one window of K iterations (at least `target` seconds) of the session `begin` opens: (K, seconds)"""
    begin()
    timed(WARM, o)
    per = timed(CALIB, o) / CALIB
    k = k_fixed or int(min(MAX_ITER - WARM - CALIB - 2, max(CALIB, np.ceil(1.15 * target / per))))    # (the first iterations run slower than the window's)
    return k, timed(k, o)


def finite_nu(o, columns):
    return all(bool(np.isfinite(o.get_scalars(o.k, rhs=j)[L.S_NU])) for j in range(columns))


result = {'workload': opt['workload'], **({} if opt['variant'] == 'hs' else {'variant': opt['variant']}), **({} if NRHS == 2 else {'nrhs': NRHS, 'knobs': KNOBS}), 'n': n, 'nnz': nnz, 'operator_bytes': op.operator_bytes(), 'window_s': window, 'repeats': repeats}
for prec in opt['prec'].split(','):
    d = 1 / A.diagonal() if prec == 'jacobi' else None
    us = {leg: [] for leg in opt['legs']}
    for rep in range(repeats):
        for leg in opt['legs']:
            o = op_c if leg == 'c' else op
            if leg in 'ac':
                k, dt = window_of(lambda: (o.begin_multi_pipe if PIPE else o.begin_multi)(VARIANT, B, X0, MAX_ITER, inv_diag=d), window, o=o)
                finite = finite_nu(o, NRHS)
            elif NRHS == 4:
                # each two-RHS session half a window: the two sessions are one window of K iterations of all four systems
                k, dt0 = window_of(lambda: op.begin_multi(VARIANT, B[:2], X0[:2], MAX_ITER, inv_diag=d), window / 2)
                finite = finite_nu(op, 2)
                _, dt1 = window_of(lambda: op.begin_multi(VARIANT, B[2:], X0[2:], MAX_ITER, inv_diag=d), window / 2, k)
                finite = finite and finite_nu(op, 2)
                dt = dt0 + dt1
            else:
                # each session half a window: the pair of sessions is one window of K iterations of both systems
                k, dt0 = window_of(lambda: op.begin(VARIANT, B[0], X0[0], MAX_ITER, inv_diag=d), window / 2)
                finite = bool(np.isfinite(op.get_scalars(op.k)[L.S_NU]))
                _, dt1 = window_of(lambda: op.begin(VARIANT, B[1], X0[1], MAX_ITER, inv_diag=d), window / 2, k)
                finite = finite and bool(np.isfinite(op.get_scalars(op.k)[L.S_NU]))
                dt = dt0 + dt1
            s = o.schedule()
            rec = {'workload': opt['workload'], 'prec': prec, 'leg': leg, 'repeat': rep, 'iterations': k, 'seconds': dt,
                   'us_per_iteration_of_both': dt / k * 1e6, 'rhs2': s.get('rhs2', False), 'rhs4': s.get('rhs4', False), 'spmm4': s.get('spmm4', False), 'rhs2_pipe': s.get('rhs2_pipe', False),
                   'window_codes': s.get('window_codes', False), 'fused': s['fused'], 'sliced_rows': s['sliced_rows'],
                   'window': s['window'], 'stream_stores': s['stream_stores'], 'finite': finite}
            print('# ' + json.dumps(rec), file=sys.stderr, flush=True)
            us[leg].append(rec['us_per_iteration_of_both'])
    out = {leg: {'median_us': float(np.median(v)), 'min_us': min(v), 'max_us': max(v)} for leg, v in us.items()}
    if 'a' in us and 'b' in us:
        out['ratio_b_over_a'] = out['b']['median_us'] / out['a']['median_us']
        spread = (out['a']['max_us'] - out['a']['min_us']) + (out['b']['max_us'] - out['b']['min_us'])
        out['a_faster_by_more_than_the_spread'] = bool(out['b']['median_us'] - out['a']['median_us'] > spread)
    if 'a' in us and 'c' in us:
        out['ratio_c_over_a'] = out['c']['median_us'] / out['a']['median_us']
        spread = (out['a']['max_us'] - out['a']['min_us']) + (out['c']['max_us'] - out['c']['min_us'])
        out['a_faster_than_c_by_more_than_the_spread'] = bool(out['c']['median_us'] - out['a']['median_us'] > spread)
    result[prec] = out
if opt['ceiling'] == '1':
    result['stream_ceiling_mode1_gbs'] = op.stream_ceiling(max(n, 1 << 20) * 4, 1)
op.close()
if op_c is not None:
    op_c.close()
print(json.dumps(result), flush=True)
