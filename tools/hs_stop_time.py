"""What the stop of a Hestenes-Stiefel single session (device.DeviceCSR.begin(L.HS, rr_stop=...); prcg.h: prcg_set_stop_hs) costs and
what it saves.
   hs_stop_time.py [workload=lap3d:128 | s4b_80 | bcsstk03 | <problems.WORKLOADS name>] [method=hs_cg | hs_pcg] [repeats=5] [iters=500]
                   [rtol=1e-8] [cap=4000] [mode=all | plain | profile] [tree=<path>]
  workload  lap3d:<m>: problems.laplace_3d(m, m, m); bcsstk03: the golden matrix (n = 112: the one-workgroup solver under hs_cg);
            anything else: problems.WORKLOADS[name].  method hs_pcg: Jacobi (inv_diag).
  mode=plain    `iters` iterations of the session WITHOUT a threshold, microseconds per iteration and iterations per second, `repeats`
                windows.  tree=<path>: import the package from that tree (the parent commit's, built): run the two alternately, process
                by process, to compare a session without a threshold against the parent.
  mode=all      (a) the CHECK: the same with rr_stop = 0 -- the stop form of every launch, nothing stops -- against the session without
                a threshold, ALTERNATING in one process;
                (b) the SAVING: the stop iteration k_stop at rtol is found first (calls of 50 iterations until the session reports it,
                at most `cap`); then ONE prcg_iterate(max_iter - 1) call + prcg_sync with max_iter = 2 k_stop -- a guessed max_iter --
                with the threshold and without, alternating, milliseconds.  The run that stops computes k_stop iterations and the
                product of the stop iteration is part of them; the other computes 2 k_stop - 1.
  mode=profile  no timing -- one session WITHOUT a threshold of 20 iterations and nothing else, for a kernel trace of what such a
                session launches (tree=<path>: the parent's, to compare the names).
Every window runs under the host clock and ends in a synchronise, after a warm-up.  Medians with each series' min and max: the
cost of the check is to be read against the spread of the windows without a threshold.  One JSON line on stdout."""
import json, os, sys, time
import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
opt = dict(workload='lap3d:128', method='hs_cg', repeats='5', iters='500', rtol='1e-8', cap='4000', mode='all', tree=HERE)
for a in sys.argv[1:]:
    k, _, v = a.partition('=')
    if k not in opt or not v:
        sys.exit(f'unknown argument {a!r}\n{__doc__}')
    opt[k] = v
if opt['method'] not in ('hs_cg', 'hs_pcg') or opt['mode'] not in ('all', 'plain', 'profile'):
    sys.exit(__doc__)
ITERS, RTOL, REPEATS, CAP = int(opt['iters']), float(opt['rtol']), int(opt['repeats']), int(opt['cap'])
WARM = 5


def series(v):
    return {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v)), 'runs': [float(q) for q in v]}


def main():
    sys.path.insert(0, opt['tree'])
    import torch  # noqa: F401
    import scipy.sparse as sp
    from new_cg_variants_amd import _lib as L
    from new_cg_variants_amd import problems as P
    from new_cg_variants_amd.device import DeviceCSR
    t0 = time.perf_counter()
    w = opt['workload']
    if w == 'bcsstk03':
        z = np.load(os.path.join(HERE, 'tests', 'golden', 'matrix_bcsstk03.npz'))
        A = sp.csr_matrix((z['data'], z['indices'], z['indptr']), shape=(int(z['n']), int(z['n'])))
        b = np.asarray(z['b'], dtype=np.float64)
    else:
        A = (P.laplace_3d(*[int(w.split(':')[1])] * 3) if w.startswith('lap3d:') else P.WORKLOADS[w]['make']()).tocsr()
        b = P.reference_rhs(A, A.shape[0])[0]
    n = A.shape[0]
    x0 = np.zeros(n)
    d = 1 / A.diagonal() if opt['method'] == 'hs_pcg' else None
    print(f'# {w} {opt["method"]}: n = {n} nnz = {A.nnz}, generated in {time.perf_counter() - t0:.1f} s', file=sys.stderr, flush=True)
    op = DeviceCSR(A)

    def begin(max_iter, rr_stop=None):
        if rr_stop is None:
            op.begin(L.HS, b, x0, max_iter, inv_diag=d)          # (the parent's begin serves this call as well)
        else:
            op.begin(L.HS, b, x0, max_iter, inv_diag=d, rr_stop=rr_stop)

    def timed(k):
        t = time.perf_counter()
        op.iterate(k)
        op.sync()
        return time.perf_counter() - t

    def per_iteration(rr_stop=None):
        begin(WARM + ITERS + 2, rr_stop)
        timed(WARM)
        return timed(ITERS) / ITERS * 1e6

    def whole_run(max_iter, rr_stop=None):
        begin(max_iter, rr_stop)
        return timed(max_iter - 1) * 1e3

    if opt['mode'] == 'profile':
        begin(22)
        timed(20)
        s = op.schedule()
        op.close()
        print(json.dumps({'workload': w, 'method': opt['method'], 'n': n, 'profile': True, 'fused': s['fused'], 'small': s['small']}), flush=True)
        return
    per_iteration()                                                # (the process's first session: clocks, caches)
    s = op.schedule()
    assert s['fused'], s
    result = {'workload': w, 'method': opt['method'], 'n': n, 'nnz': int(A.nnz), 'iters': ITERS, 'repeats': REPEATS, 'rtol': RTOL,
              'small': s['small'], 'window': s['window'], 'sliced_rows': s['sliced_rows'], 'tree': 'this' if opt['tree'] == HERE else opt['tree']}
    if opt['mode'] == 'plain':
        plain = [per_iteration() for _ in range(REPEATS)]
        result.update(plain_us=series(plain), plain_it_per_s=1e6 / float(np.median(plain)))
        op.close()
        print(json.dumps(result), flush=True)
        return
    plain, zero = [], []
    for _ in range(REPEATS):
        plain.append(per_iteration())
        zero.append(per_iteration(0.0))
        assert op.stop() == (-1, 0), op.stop()
    result.update(plain_us=series(plain), zero_us=series(zero), plain_it_per_s=1e6 / float(np.median(plain)))
    result['a_check_cost'] = result['zero_us']['median'] / result['plain_us']['median']
    result['a_check_exceeds_plain_spread'] = bool(result['zero_us']['median'] > result['plain_us']['max'])
    # (b) where does the session stop at rtol?
    thr = float((RTOL * np.linalg.norm(b)) ** 2)
    begin(CAP, thr)
    while op.k < CAP - 1 and op.stop()[0] < 0:
        op.iterate(min(50, CAP - 1 - op.k))
    k_stop, status = op.stop()
    result.update(thr=thr, k_stop=k_stop, status=status)
    if status and k_stop > 0:
        result['rr_at_stop'] = float(op.get_scalars(k_stop)[L.S_RR])
        max_iter = 2 * k_stop
        free_ms, stop_ms = [], []
        for _ in range(REPEATS):
            free_ms.append(whole_run(max_iter))
            stop_ms.append(whole_run(max_iter, thr))
            assert op.stop() == (k_stop, status), (op.stop(), k_stop, status)
        result.update(max_iter=max_iter, plain_run_ms=series(free_ms), stop_run_ms=series(stop_ms))
        result['b_stop_run_vs_plain_run'] = result['stop_run_ms']['median'] / result['plain_run_ms']['median']
    op.close()
    print(json.dumps(result), flush=True)


if __name__ == '__main__':
    main()
