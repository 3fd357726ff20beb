"""TEST INFRASTRUCTURE of tests/test_single_stop.py: the oracle's free-running trajectory of a pipelined single session under a
given summation order, the stopping rule applied to it in Python (the test's own restatement, as small_batch_common.rule is the
batch's), and one device session read back in full."""
import numpy as np

from small_batch_common import BREAKDOWN, CONVERGED, rule          # noqa: F401 -- the rule is the batch's

# method -> (device variant, the oracle's flavour, Jacobi)
METHODS = {
    'pipe_pr_cg': ('PIPE_PR', 'pr', False), 'pipe_pr_pcg': ('PIPE_PR', 'pr', True),
    'pipe_pr_m_cg': ('PIPE_PR_M', 'pr_m', False), 'pipe_pr_m_pcg': ('PIPE_PR_M', 'pr_m', True),
    'pipe_p_cg': ('PIPE_P', 'p', False), 'pipe_p_pcg': ('PIPE_P', 'p', True),
}


def vectors_of(method):
    """the state a stopped session holds (prcg.h: prcg_set_stop): x, r, p, s, w, u; with Jacobi r~ and s~; the 'p' flavours
    with Jacobi also their stored w~"""
    _, flavour, jac = METHODS[method]
    return ('x', 'r', 'p', 's', 'w', 'u') + (('rt', 'st') if jac else ()) + (('wt',) if jac and flavour == 'p' else ())


def trajectory(A, b, method, dot, dot0, iters, keep=None, x0=None):
    """The oracle (oracle/ne_oracle.py: pipe_start / pipe_advance) from x0 (None: zeros), `iters` iterations, NO stopping: row k of
    `scalars` = {mu, delta, gamma, nu, rr} of state k (rr = r.r summed like the others: row 0 by dot0, the start-up launch's
    order, later rows by dot, the iteration launch's), row k - 1 of `coef` = {a, b, predicted nu} of iteration k, `at[k]` the
    vectors of state k (keep: only at those k, None elsewhere; default every k).  A breakdown leaves inf / nan behind, as the
    reference does."""
    import oracle.ne_oracle as O
    _, flavour, jac = METHODS[method]
    prec = O.jacobi(A) if jac else None
    names = vectors_of(method)
    plain, plain0 = dot, dot0

    def dot(a, b):              # (not a Python float: nu / mu must give inf / nan at a breakdown, not raise)
        return np.float64(plain(a, b))

    def dot0(a, b):
        return np.float64(plain0(a, b))

    def snap(st):
        if keep is not None and st.k not in keep:
            return None
        return {v: np.array(getattr(st, v), copy=True) for v in names}
    with np.errstate(all='ignore'):
        st = O.pipe_start(A, b, np.zeros(b.size) if x0 is None else x0, prec=prec, dot=dot0)
        scalars, coef, at = [[st.mu, st.dl, st.gm, st.nu, dot0(st.r, st.r)]], [], [snap(st)]
        for _ in range(iters):
            a = st.alpha
            O.pipe_advance(A, st, flavour=flavour, prec=prec, dot=dot, square=lambda q: q * q)
            coef.append([a, st.beta, st.nu_pred])
            scalars.append([st.mu, st.dl, st.gm, st.nu, dot(st.r, st.r)])
            at.append(snap(st))
    return dict(scalars=np.array(scalars, dtype=np.float64), coef=np.array(coef, dtype=np.float64).reshape(-1, 3), at=at)


def stop_of(traj, thr):
    """(k_stop, status) of the rule on the trajectory's rows: the first k it fires at, or (-1, 0)"""
    for k, (mu, _, _, nu, rr) in enumerate(traj['scalars']):
        status = rule(mu, nu, rr, thr)
        if status:
            return k, status
    return -1, 0


def run_session(L, op, method, b, inv_diag, max_iter, rr_stop, chunks, then=0, x0=None):
    """one device session from x0 (None: zeros) with the recurrence residual recorded: prcg_iterate calls of `chunks` WITHOUT a
    synchronisation between them, then prcg_sync; everything the session holds is read back.  then > 0: a further
    prcg_iterate(then) and a second reading (`again`).  With an x0, x and r are also read right after begin (`start`)."""
    variant = getattr(L, METHODS[method][0])
    names = vectors_of(method)
    op.begin(variant, b, np.zeros(b.size) if x0 is None else x0, max_iter, inv_diag=inv_diag, hist_mask=1, rr_stop=rr_stop)
    out = {'schedule': op.schedule(), 'start_layout': op.layout()}
    if x0 is not None:
        out['start'] = (op.get_vector('x'), op.get_vector('r'))
    for c in chunks:
        op.iterate(c)
    op.sync()

    def read():
        return dict(k=int(op.k), stop=op.stop(), at={v: op.get_vector(v) for v in names},
                    scalars=np.array([op.get_scalars(k) for k in range(max_iter)]),
                    coef=np.array([op.get_coefficients(k) for k in range(1, max_iter)]).reshape(-1, 3),
                    hist=op.history()['updated_residual_2_norm'])
    out.update(read())
    out['layout'] = op.layout()
    if then:
        op.iterate(then)
        op.sync()
        out['again'] = read()
    return out


def same_reading(a, b):
    return a['k'] == b['k'] and a['stop'] == b['stop'] and all(np.array_equal(a['at'][v], b['at'][v], equal_nan=True) for v in a['at']) and \
        np.array_equal(a['scalars'], b['scalars'], equal_nan=True) and np.array_equal(a['coef'], b['coef'], equal_nan=True) and \
        np.array_equal(a['hist'], b['hist'], equal_nan=True)


def holds_trajectory(rec, traj, k_stop, status, max_iter, what=''):
    """a device reading against the oracle's trajectory stopped at k_stop (status 0: ran to the end, k_stop = max_iter - 1)"""
    last = k_stop if status else max_iter - 1
    assert rec['stop'] == ((k_stop, status) if status else (-1, 0)), (what, 'stop word', rec['stop'], (k_stop, status))
    assert rec['k'] == last, (what, 'prcg_iteration after prcg_sync', rec['k'], last)
    for v, want in traj['at'][last].items():
        differ = int(np.count_nonzero(~(rec['at'][v] == want)))
        assert differ == 0, (what, f'{v} at k={last}: {differ} of {want.size} entries differ')
    assert rec['scalars'].shape == (max_iter, 8) and rec['coef'].shape == (max_iter - 1, 3) and rec['hist'].shape == (max_iter,)
    got, want = rec['scalars'][:last + 1, :5], traj['scalars'][:last + 1]
    bad = ~(got == want)
    assert not bad.any(), (what, f'scalars: first mismatch at k={int(np.argmax(bad.any(axis=1)))}', got[bad.any(axis=1)][:1], want[bad.any(axis=1)][:1])
    assert np.array_equal(rec['scalars'][:last + 1, 5:], np.zeros((last + 1, 3))), (what, 'recorder slots nobody asked for')
    bad = ~(rec['coef'][:last] == traj['coef'][:last])
    assert not bad.any(), (what, f'coefficients: first mismatch at k={int(np.argmax(bad.any(axis=1))) + 1}')
    assert np.array_equal(rec['scalars'][last + 1:], np.zeros((max_iter - 1 - last, 8))), (what, 'scalar rows beyond the stop')
    assert np.array_equal(rec['coef'][last:], np.zeros((max_iter - 1 - last, 3))), (what, 'coefficient rows beyond the stop')
    assert np.array_equal(rec['hist'][:last + 1], np.sqrt(traj['scalars'][:last + 1, 4])), (what, 'history')
    assert np.array_equal(rec['hist'][last + 1:], np.zeros(max_iter - 1 - last)), (what, 'history beyond the stop')
