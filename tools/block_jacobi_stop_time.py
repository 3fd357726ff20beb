"""What the stop of a pipelined single session with point-block Jacobi (device.DeviceCSR.begin(block_jacobi= | block_jacobi_var=,
rr_stop=...); prcg.h: prcg_set_stop_block_jacobi) costs and what it saves, under pipe_pr's session (PRCG_PIPE_PR).
   block_jacobi_stop_time.py [workload=s4b_80 | fem:<m> | irr:<m>] [repeats=7] [iters=500] [rtol=1e-8] [cap=4000] [profile=0] [tree=<path>]
  workload  s4b_80: problems.WORKLOADS['s4b_80'] with blocks of 3 built on the device (DeviceBlockJacobi(A, 3)); fem:<m>: fem_like_3d(m, 3),
            the same at another size;
            irr:<m>: problems.fem_irregular_3d(m) with its nodal partition, built on the device (irr:80 is the measured one)
  (a) the CHECK: `iters` iterations of the session with rr_stop = 0 -- the stop form of every launch, nothing stops -- against the
      same session without a threshold, microseconds per iteration, ALTERNATING in one process, `repeats` windows each;
  (b) the SAVING: the stop iteration k_stop at rtol is found first (calls of 50 iterations until the session reports it, at most
      `cap`); then ONE prcg_iterate(max_iter - 1) call + prcg_sync with max_iter = 2 k_stop, with the threshold and without,
      alternating, milliseconds.
  profile=1: no timing -- one session WITHOUT a threshold of 20 iterations and nothing else, for a kernel trace of what such a
      session launches.  tree=<path>: import the package from that tree (the parent commit's, built), to compare the names.
Every window runs under the host clock and ends in a synchronise, after a warm-up session.  Medians with each series' min and
max: the cost of the check is to be read against the spread of the windows without a threshold.  One JSON line on stdout."""
import json, os, sys, time
import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
opt = dict(workload='s4b_80', repeats='7', iters='500', rtol='1e-8', cap='4000', profile='0', tree=HERE)
for a in sys.argv[1:]:
    k, _, v = a.partition('=')
    if k not in opt or not v:
        sys.exit(f'unknown argument {a!r}\n{__doc__}')
    opt[k] = v
ITERS, RTOL, REPEATS, CAP = int(opt['iters']), float(opt['rtol']), int(opt['repeats']), int(opt['cap'])
WARM = 5


def series(v):
    return {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v)), 'runs': [float(q) for q in v]}


def main():
    sys.path.insert(0, opt['tree'])
    import torch  # noqa: F401
    from new_cg_variants_amd import _lib as L
    from new_cg_variants_amd import problems as P
    from new_cg_variants_amd.device import DeviceCSR
    t0 = time.perf_counter()
    if opt['workload'].startswith('irr:'):
        m = int(opt['workload'].split(':')[1])
        A = P.fem_irregular_3d(m).tocsr()
        blocks = {'block_jacobi_var': (P.fem_irregular_blocks(m), None)}
    else:
        A = (P.fem_like_3d(int(opt['workload'].split(':')[1]), 3) if opt['workload'].startswith('fem:') else P.WORKLOADS[opt['workload']]['make']()).tocsr()
        blocks = {'block_jacobi': (3, None)}
    n = A.shape[0]
    b = P.reference_rhs(A, n)[0]
    x0 = np.zeros(n)
    print(f'# {opt["workload"]}: n = {n} nnz = {A.nnz}, generated in {time.perf_counter() - t0:.1f} s', file=sys.stderr, flush=True)
    op = DeviceCSR(A)

    def begin(max_iter, rr_stop=None):
        op.begin(L.PIPE_PR, b, x0, max_iter, rr_stop=rr_stop, **blocks)

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

    if opt['profile'] != '0':
        op.begin(L.PIPE_PR, b, x0, 22, **blocks)
        timed(20)
        s = op.schedule()
        op.close()
        print(json.dumps({'workload': opt['workload'], 'n': n, 'profile': True, 'block_jacobi': s['block_jacobi'], 'fused': s['fused']}), flush=True)
        return
    per_iteration()                                                # (the process's first session: clocks, caches, the blocks' build)
    s = op.schedule()
    assert s['block_jacobi'] and not s['fused'] and not s['small'], s
    plain, zero = [], []
    for _ in range(REPEATS):
        plain.append(per_iteration())
        zero.append(per_iteration(0.0))
        assert op.stop() == (-1, 0), op.stop()
    result = {'workload': opt['workload'], 'n': n, 'nnz': int(A.nnz), 'iters': ITERS, 'repeats': REPEATS, 'rtol': RTOL,
              'plain_us': series(plain), 'zero_us': series(zero)}
    result['a_check_cost'] = result['zero_us']['median'] / result['plain_us']['median']
    result['a_check_exceeds_plain_spread'] = bool(result['zero_us']['median'] > result['plain_us']['max'])
    # (b) where does the session stop at rtol?
    thr = float((RTOL * np.linalg.norm(b)) ** 2)
    begin(CAP, thr)
    while op.k < CAP - 1 and op.stop()[0] < 0:
        op.iterate(min(50, CAP - 1 - op.k))
    k_stop, status = op.stop()
    result.update(thr=thr, k_stop=k_stop, status=status)
    if status:
        result['rr_at_stop'] = float(op.get_scalars(k_stop)[L.S_RR])
        max_iter = max(2 * k_stop, 2)
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
