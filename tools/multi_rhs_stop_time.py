"""What the per-column stop of the pipelined two-RHS session (device.DeviceCSR.begin_multi_pipe(rr_stop=...): each column stops at
its own threshold on r.r, decided on the device) costs and what it saves, under Jacobi pipe_pr_pcg_multi's session, against the
PARENT commit's tree in the same sitting.
   multi_rhs_stop_time.py [workload=s4b_80 | lap3d:<nx>] [parent=<path of the parent commit's tree, built>] [repeats=5]
                          [iters=200] [max_iter=600] [rtol=1e-8]
  (a) the CHECK: `iters` iterations of the session with thresholds (0, 0) -- the stop forms of every kernel, nothing stops --
      against the same session without thresholds, microseconds per iteration of both systems;
  (b) the SAVING: ONE prcg_iterate(max_iter - 1) call + prcg_sync of the session with rtol (thr_c = (rtol ||b_c||)^2), which stops
      both columns, against the session without thresholds run to max_iter;
  (c) the iteration time while ONE column is frozen: thresholds (1e300, 0) stop column 0 on the initial state, (0, 1e300) column 1.
The driver builds the operator once, writes its CSR arrays to a scratch directory and starts a FRESH process per run, alternating
this tree and the parent's (which imports its own package and library and runs the two legs it has: the session without
thresholds per iteration and run to max_iter); `repeats` runs each.  Every leg: a window under the host clock that ends in a
synchronise, after a warm-up.  The medians are reported with each series' min and max: this tree's session without thresholds
must be read against the parent's own spread.  lap3d:<nx> is laplace_3d(nx, nx, nx): a window operator (two two-vector
products per iteration); s4b_80 runs on sliced rows (the one four-vector product).
One record per run on stderr, ONE JSON line on stdout."""
import json, os, subprocess, sys, tempfile, time
import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
opt = dict(workload='s4b_80', parent='', repeats='5', iters='200', max_iter='600', rtol='1e-8', child='', tree=HERE, legs='all')
for a in sys.argv[1:]:
    k, _, v = a.partition('=')
    if k not in opt or not v:
        sys.exit(f'unknown argument {a!r}\n{__doc__}')
    opt[k] = v
ITERS, MAX_ITER, RTOL, REPEATS = int(opt['iters']), int(opt['max_iter']), float(opt['rtol']), int(opt['repeats'])
WARM = 5


def child():
    """one run in a process of its own: the tree named by tree=, the operator from the arrays under child="""
    sys.path.insert(0, opt['tree'])
    import scipy.sparse as sp
    import torch  # noqa: F401
    from new_cg_variants_amd import _lib as L
    from new_cg_variants_amd.device import DeviceCSR
    d_ = opt['child']
    indptr, indices, data = (np.load(os.path.join(d_, q + '.npy')) for q in ('indptr', 'indices', 'data'))
    n = indptr.size - 1
    A = sp.csr_matrix((data, indices, indptr), shape=(n, n))
    B, X0 = np.load(os.path.join(d_, 'B.npy')), np.zeros((2, n))
    inv_diag = 1 / A.diagonal()
    op = DeviceCSR(A)

    def begin(max_iter, rr_stop=None):
        kw = {} if rr_stop is None else {'rr_stop': rr_stop}
        op.begin_multi_pipe(L.PIPE_PR, B, X0, max_iter, inv_diag=inv_diag, **kw)

    def timed(k):
        t = time.perf_counter()
        op.iterate(k)
        op.sync()
        return time.perf_counter() - t

    def per_iteration(rr_stop=None):
        begin(WARM + ITERS + 2, rr_stop)
        timed(WARM)
        return timed(ITERS) / ITERS * 1e6

    def whole_run(rr_stop=None):
        begin(MAX_ITER, rr_stop)
        return timed(MAX_ITER - 1) * 1e3

    rec = {'tree': opt['tree'], 'n': n, 'nnz': int(A.nnz)}
    per_iteration()                                            # (the process's first session: clocks, caches, placement)
    rec['plain_us'] = per_iteration()
    rec['plain_run_ms'] = whole_run()
    rec['spmm4'] = op.schedule()['spmm4']
    if opt['legs'] == 'all':
        rec['zero_us'] = per_iteration([0.0, 0.0])
        rec['zero_stops'] = op.stops_rhs()
        thr = [(RTOL * np.linalg.norm(b)) ** 2 for b in B]
        rec['stop_run_ms'] = whole_run(thr)
        rec['stops'] = op.stops_rhs()
        rec['rr_at_stop'] = [float(op.get_scalars(max(k, 0), rhs=c)[L.S_RR]) for c, (k, _) in enumerate(rec['stops'])]
        rec['thr'] = thr
        rec['frozen0_us'] = per_iteration([1e300, 0.0])
        rec['frozen0_stops'] = op.stops_rhs()
        rec['frozen1_us'] = per_iteration([0.0, 1e300])
        rec['frozen1_stops'] = op.stops_rhs()
        rec['plain_again_us'] = per_iteration()
    op.close()
    print(json.dumps(rec), flush=True)


def series(v):
    return {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v)), 'runs': [float(q) for q in v]}


def driver():
    sys.path.insert(0, HERE)
    from new_cg_variants_amd import problems as P
    t0 = time.perf_counter()
    if opt['workload'].startswith('lap3d:'):
        nx = int(opt['workload'].split(':')[1])
        A = P.laplace_3d(nx, nx, nx)
    else:
        A = P.WORKLOADS[opt['workload']]['make']()
    A = A.tocsr()
    n = A.shape[0]
    B = np.stack([P.reference_rhs(A, n)[0], np.random.default_rng(7).standard_normal(n)])
    print(f'# {opt["workload"]}: n = {n} nnz = {A.nnz}, generated in {time.perf_counter() - t0:.1f} s', file=sys.stderr, flush=True)
    runs = {'this': [], 'parent': []}
    with tempfile.TemporaryDirectory() as d_:
        for q, v in (('indptr', A.indptr), ('indices', A.indices), ('data', A.data), ('B', B)):
            np.save(os.path.join(d_, q + '.npy'), v)
        del A
        for rep in range(REPEATS):
            for who, tree in (('this', HERE), ('parent', opt['parent'])):
                if not tree:
                    continue
                env = dict(os.environ)
                env.pop('PRCG_LIB', None)
                cmd = [sys.executable, os.path.join(HERE, 'tools', 'multi_rhs_stop_time.py'), f'child={d_}', f'tree={tree}',
                       f'legs={"all" if who == "this" else "plain"}', f'iters={ITERS}', f'max_iter={MAX_ITER}', f'rtol={RTOL}']
                out = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=600)
                if out.returncode != 0:
                    sys.exit(f'the run of {who} (repeat {rep}) ended with status {out.returncode}: nothing more is started')
                rec = json.loads(out.stdout.strip().splitlines()[-1])
                rec.update(who=who, repeat=rep)
                print('# ' + json.dumps(rec), file=sys.stderr, flush=True)
                runs[who].append(rec)
    mine = runs['this']
    result = {'workload': opt['workload'], 'n': n, 'iters': ITERS, 'max_iter': MAX_ITER, 'rtol': RTOL, 'repeats': REPEATS, 'spmm4': mine[0]['spmm4'],
              'this': {q: series([r[q] for r in mine]) for q in ('plain_us', 'plain_again_us', 'zero_us', 'frozen0_us', 'frozen1_us', 'plain_run_ms', 'stop_run_ms')},
              'stops': mine[-1]['stops'], 'thr': mine[-1]['thr'], 'rr_at_stop': mine[-1]['rr_at_stop'], 'zero_stops': mine[-1]['zero_stops'],
              'frozen0_stops': mine[-1]['frozen0_stops'], 'frozen1_stops': mine[-1]['frozen1_stops']}
    t = result['this']
    result['a_check_cost'] = t['zero_us']['median'] / t['plain_us']['median']
    result['b_stop_run_vs_plain_run'] = t['stop_run_ms']['median'] / t['plain_run_ms']['median']
    if runs['parent']:
        p = {q: series([r[q] for r in runs['parent']]) for q in ('plain_us', 'plain_run_ms')}
        result['parent'] = p
        result['plain_inside_parent_spread'] = bool(p['plain_us']['min'] <= t['plain_us']['median'] <= p['plain_us']['max'])
        result['a_check_cost_vs_parent'] = t['zero_us']['median'] / p['plain_us']['median']
        result['a_check_exceeds_parent_spread'] = bool(t['zero_us']['median'] > p['plain_us']['max'])
        result['b_stop_run_vs_parent_plain_run'] = t['stop_run_ms']['median'] / p['plain_run_ms']['median']
    print(json.dumps(result), flush=True)


if __name__ == '__main__':
    child() if opt['child'] else driver()
