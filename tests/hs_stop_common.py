"""TEST INFRASTRUCTURE of tests/test_hs_stop.py and tests/test_hs_stop_model.py: the oracle's free-running hs_cg / hs_pcg trajectory
under a given summation order, read from its tap; the stopping rule applied to its rows in Python (single_stop_common.stop_of:
small_batch_common.rule, the batch's); one device Hestenes-Stiefel session read back in full; the cases.

Which launch sums which inner product (tests/test_trajectory_oracle.py, tests/test_trajectory_irregular.py): the oracle asks for
nu, then mu, in its start and in every advance (device_order.Routed).  Iterations: nu by launch_hs_update_xr (pair tree), mu by the
product launch (tile / unit tree of the layout the session reports); the one-workgroup solver sums both in its own order
(small_batch_common.wg_sum).  Start-up, every schedule: nu by launch_hs_init_dots (pair tree), mu by the start-up product (the tree
of the layout right after begin).  rr = r.r is summed like nu -- by the same launch, element by element beside it; without a
preconditioner it IS nu."""
import numpy as np

from single_stop_common import holds_trajectory, same_reading, stop_of          # noqa: F401 -- rows {mu, -, -, nu, rr} fit them as they are
from small_batch_common import BREAKDOWN, CONVERGED, rule                        # noqa: F401

METHODS = {'hs_cg': False, 'hs_pcg': True}         # method -> Jacobi

# operator -> (knobs of the handle, family the schedule must report)
OPERATORS = {
    's3_small': ({'PRCG_SMALL': '0'}, 'window'), 's1_small': ({'PRCG_SMALL': '0'}, 'window'), 'lap3d': ({'PRCG_SMALL': '0'}, 'window'),
    'fem12': ({}, 'sell_win'), 'irr10': ({'PRCG_SELL_WINDOW': '0'}, 'sell'), 'bcsstk14': ({'PRCG_SELL': '0'}, 'csr'),
    'bcsstk03_wg': ({}, 'small'), 'nos4_wg': ({}, 'small'), 'lap27_wg': ({}, 'small'), 'lap1d_wg': ({}, 'small'),
    # s1_small with default knobs was meant for the one-workgroup solver (n = 3072: three rows per thread), but its matrix does not fit
    # beside the vectors (small_lds_bytes: 280 KB against the 156 KB cap), so the session runs on window tiles -- kept as the case it
    # is; laplace_2d(2100, 1) (n = 2100, 6298 nonzeros, 140 KB) is the system that does run there with three rows per thread
    's1_small_default': ({}, 'window'),
    'lap2d_indef': ({'PRCG_SMALL': '0'}, 'window'), 'lap27_indef': ({}, 'small'),
}
# (operator, method, max_iter): under np.dot every one stops at max_iter // 2 with thr = rr there -- except bcsstk03 (its residual
# is not monotone: the first k with rr <= rr[20] is 16)
CASES = [('s3_small', 'hs_cg', 10), ('s3_small', 'hs_pcg', 5), ('s1_small', 'hs_cg', 10), ('s1_small', 'hs_pcg', 10),
         ('lap3d', 'hs_cg', 10), ('lap3d', 'hs_pcg', 10), ('fem12', 'hs_cg', 32), ('fem12', 'hs_pcg', 24),
         ('irr10', 'hs_cg', 48), ('irr10', 'hs_pcg', 24), ('bcsstk14', 'hs_cg', 10), ('bcsstk14', 'hs_pcg', 10),
         ('bcsstk03_wg', 'hs_cg', 40), ('nos4_wg', 'hs_cg', 40), ('lap27_wg', 'hs_cg', 30), ('s1_small_default', 'hs_cg', 10),
         ('lap1d_wg', 'hs_cg', 10)]
# (operator, method, max_iter, k of the breakdown): symmetric indefinite operators, thr = 1e-300
BREAKDOWNS = [('lap2d_indef', 'hs_cg', 30, 19), ('lap2d_indef', 'hs_pcg', 30, 19), ('lap27_indef', 'hs_cg', 30, 14)]
GOLDEN = {'bcsstk14': 'bcsstk14', 'bcsstk03_wg': 'bcsstk03', 'nos4_wg': 'nos4'}


def case_id(c):
    return '-'.join(str(q) for q in c)


def make_problem(P, matrices):
    """operator -> (A, b, inverse diagonal), built once and left unchanged; rhs 'zero': b = 0"""
    import scipy.sparse as sp
    make = {'s3_small': lambda: P.WORKLOADS['s3_small']['make'](), 's1_small': lambda: P.WORKLOADS['s1_small']['make'](),
            's1_small_default': lambda: P.WORKLOADS['s1_small']['make'](), 'lap1d_wg': lambda: P.laplace_2d(2100, 1), 'lap3d': lambda: P.laplace_3d(21, 17, 13),
            'fem12': lambda: P.fem_like_3d(12), 'irr10': lambda: P.fem_irregular_3d(10), 'lap27_wg': lambda: P.laplace_2d(27, 27),
            'lap2d_indef': lambda: P.laplace_2d(64, 48) - 0.02 * sp.identity(64 * 48),
            'lap27_indef': lambda: P.laplace_2d(27, 27) - 0.05 * sp.identity(27 * 27)}
    cache = {}

    def get(operator, rhs='ref'):
        if operator not in cache:
            if operator in make:
                A = sp.csr_matrix(make[operator]())
                b = P.reference_rhs(A, A.shape[0])[0]
            else:
                A, z = matrices[GOLDEN[operator]]
                b = np.asarray(z['b'], dtype=np.float64)
            cache[operator] = (A, b, 1 / A.diagonal())
        A, b, d = cache[operator]
        return (A, np.zeros(A.shape[0]), d) if rhs == 'zero' else (A, b, d)
    return get


def vectors_of(method):
    """the state a stopped session holds (prcg.h: prcg_set_stop_hs): x, r, p, s; with Jacobi r~"""
    return ('x', 'r', 'p', 's') + (('rt',) if METHODS[method] else ())


def _trajectory(A, b, method, dot, dot0, rr_of, iters, keep, x0):
    import oracle.ne_oracle as O
    names = vectors_of(method)
    scalars, alphas, betas, at = [], [], [], []

    def tap(st):
        scalars.append([st.mu, 0.0, 0.0, st.nu, rr_of(st.k, st.r)])
        alphas.append(st.alpha)
        betas.append(st.beta)
        at.append({v: np.array(getattr(st, v), copy=True) for v in names} if keep is None or st.k in keep else None)
    kw = {'preconditioner': O.jacobi(A)} if METHODS[method] else {}
    with np.errstate(all='ignore'):
        getattr(O, method)(A, b, np.zeros(b.size) if x0 is None else x0, iters + 1, dot=dot, dot0=dot0, tap=tap, **kw)
    coef = np.zeros((iters, 3))
    coef[:, 0], coef[:, 1] = alphas[:-1], betas[1:]          # a of iteration k: the step state k - 1 holds; b: what state k used
    return dict(scalars=np.array(scalars, dtype=np.float64), coef=coef, at=at)


def trajectory(A, b, method, sums, sums0, iters, keep=None, x0=None):
    """The oracle's hs_cg / hs_pcg (oracle/ne_oracle.py) from x0 (None: zeros), `iters` iterations, NO stopping, read from its tap.
    sums = (nu's sum, mu's sum) of the iterations, sums0 of the start-up: callables on the array of products.  Row k of `scalars` =
    {mu, 0, 0, nu, rr} of state k (rr by nu's sum), row k - 1 of `coef` = {a, b, 0} of iteration k, `at[k]` the vectors of state k
    (keep: only at those k, None elsewhere; default every k).  A breakdown leaves inf / nan behind, as the reference does."""
    from device_order import Routed
    return _trajectory(A, b, method, Routed(*sums), Routed(*sums0), lambda k, r: np.float64((sums0 if k == 0 else sums)[0](r * r)), iters, keep, x0)


def trajectory_np(A, b, method, iters, keep=None):
    """the same rows under np.dot: the CPU model of tests/test_hs_stop_model.py, which has no device order to follow"""
    return _trajectory(A, b, method, np.dot, np.dot, lambda k, r: np.dot(r, r), iters, keep, None)


def run_session(L, op, method, b, inv_diag, max_iter, rr_stop, chunks, then=0):
    """one device session from x0 = 0 with the recurrence residual recorded: prcg_iterate calls of `chunks` WITHOUT a
    synchronisation between them, then prcg_sync; everything the session holds is read back.  then > 0: a further
    prcg_iterate(then) and a second reading (`again`)."""
    names = vectors_of(method)
    op.begin(L.HS, b, np.zeros(b.size), max_iter, inv_diag=inv_diag, hist_mask=1, rr_stop=rr_stop)
    out = {'schedule': op.schedule(), 'start_layout': op.layout()}
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


def oracle_sums(A, operator, jac, rec):
    """the schedule the case is there for, from the flags and tables the session reports; returns (sums, sums0) for `trajectory`"""
    from device_order import OneLaunchTree, UnitTree, pair_sum, tile_cap_nnz
    from small_batch_common import wg_sum
    s, lay, lay0 = rec['schedule'], rec['layout'], rec['start_layout']
    family = OPERATORS[operator][1]
    if family == 'small' and jac:
        family = 'window'                  # (a Jacobi single session does not select the one-workgroup solver: window tiles)
    assert s['fused'] and not s['comm'] and not s['fused_comm'] and not s['block_jacobi'], s
    assert s['small'] == (family == 'small'), s
    assert lay0['grid'] > 0 and lay['grid'] > 0, (lay0['grid'], lay['grid'])

    def tree(layout):
        if layout['window']:
            return OneLaunchTree(layout)
        return UnitTree.of(layout)
    sums0 = (pair_sum, tree(lay0).sum)
    if family == 'small':
        return (wg_sum, wg_sum), sums0
    assert s['window'] == (family == 'window') and lay['window'] == s['window'], s
    assert s['sliced_rows'] == (family in ('sell', 'sell_win')) and lay['sliced'] == s['sliced_rows'], s
    if s['sliced_rows']:
        assert s['window_codes'] == (family == 'sell_win'), s                 # k_sell_win / k_sell_tiles
    elif not s['window']:
        assert np.diff(A.indptr).max() <= tile_cap_nnz(s['tile_steps'])       # no long rows: SciPy's product is the device's
    return (pair_sum, tree(lay).sum), sums0


def same_launch(a, b):
    return a['layout']['grid'] == b['layout']['grid'] and a['layout']['waves_per_block'] == b['layout']['waves_per_block']
