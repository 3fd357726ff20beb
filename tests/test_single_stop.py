"""A pipelined SINGLE session stops at a residual threshold, decided on the device (prcg.h: prcg_set_stop, prcg_get_stop;
device.DeviceCSR.begin(rr_stop=...), .stop(); cg_variants.pipe_*(rtol=, atol=)).

The yardstick is the oracle's free-running trajectory under the device's own summation order, as tests/test_trajectory_oracle.py
and tests/test_trajectory_irregular.py build it (OneLaunchTree for window operators, UnitTree for sliced rows and CSR-adaptive
tiles, from the layout the session reports; the one-workgroup solver: small_batch_common.wg_dot), with the stopping rule
applied to its rows in Python (single_stop_common.stop_of: small_batch_common.rule, the batch's).  Everything is compared for
equal bits.  Thresholds come from the oracle: thr = its rr at iteration max_iter // 2; the stop is the first k the rule fires at.

Run lengths (max_iter) are chosen per case so that 0 < k_stop < max_iter - 1 and the run does not break down before its end
(the thr = 0 comparison needs that) -- found on the CPU with the oracle, asserted here again under the device's tree:
 * fem_like_3d(12), fem_irregular_3d(10) without a preconditioner: the residual first GROWS (rr at 12 above rr at 0): 32 / 48;
 * s3_small with Jacobi converges in four iterations and pipe_pr_m_pcg breaks down at k = 6: 5 / 6;
 * nos7 without a preconditioner (the one-workgroup solver) on the fixture's right-hand side never gets below its initial rr
   within 3000 iterations: the cases use a random right-hand side for pipe_pr_cg (400 iterations: k_stop = 200) and ones for
   pipe_pr_m_cg (800: k_stop = 369).
Breakdown on the one-workgroup path: nos7 under pipe_pr_cg does NOT break down -- the oracle under the workgroup's order was run
for 40 000 iterations on the fixture's right-hand side and 3000 on three others, the recurrence residual just keeps shrinking
(rr = 1e-165 at k = 39 945) -- so that case takes an indefinite operator of nos7's size, laplace_2d(27, 27) - 0.05 I (k = 14)."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from device_order import OneLaunchTree, UnitTree, device_dot, tile_cap_nnz
from single_stop_common import BREAKDOWN, CONVERGED, METHODS, holds_trajectory, run_session, same_reading, stop_of, trajectory
from small_batch_common import wg_dot

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PIPELINED = ['pipe_pr_cg', 'pipe_pr_m_cg', 'pipe_p_cg', 'pipe_p_m_cg', 'pipe_pr_pcg', 'pipe_pr_m_pcg', 'pipe_p_pcg', 'pipe_p_m_pcg']

# operator -> (knobs of the handle, family the schedule must report)
OPERATORS = {
    's3_small': ({'PRCG_SMALL': '0'}, 'window'), 's1_small': ({'PRCG_SMALL': '0'}, 'window'), 'lap3d': ({'PRCG_SMALL': '0'}, 'window'),
    'fem12': ({'PRCG_SMALL': '0'}, 'sell_win'), 'irr10': ({'PRCG_SMALL': '0', 'PRCG_SELL_WINDOW': '0'}, 'sell'),
    'bcsstk14': ({'PRCG_SMALL': '0', 'PRCG_SELL': '0'}, 'csr'),
    'nos7': ({}, 'small'),              # (with Jacobi a single session takes the one-launch path: window tiles)
    'lap2d_indef': ({'PRCG_SMALL': '0'}, 'window'), 'lap27_indef': ({}, 'small'),
}
# (operator, method, right-hand side, max_iter): module docstring
CASES = [(o, m, 'ref', 10) for o in ('s3_small', 's1_small', 'lap3d', 'bcsstk14') for m in ('pipe_pr_cg', 'pipe_pr_m_cg')] + \
        [(o, m, 'ref', 10) for o in ('s1_small', 'lap3d', 'bcsstk14', 'nos7') for m in ('pipe_pr_pcg', 'pipe_pr_m_pcg')] + \
        [('s3_small', 'pipe_pr_pcg', 'ref', 6), ('s3_small', 'pipe_pr_m_pcg', 'ref', 5), ('s3_small', 'pipe_p_cg', 'ref', 10),
         ('s3_small', 'pipe_p_pcg', 'ref', 6)] + \
        [('fem12', m, 'ref', 32) for m in ('pipe_pr_cg', 'pipe_pr_m_cg', 'pipe_p_cg')] + \
        [('fem12', m, 'ref', 24) for m in ('pipe_pr_pcg', 'pipe_pr_m_pcg', 'pipe_p_pcg')] + \
        [('irr10', m, 'ref', 48) for m in ('pipe_pr_cg', 'pipe_pr_m_cg')] + [('irr10', m, 'ref', 24) for m in ('pipe_pr_pcg', 'pipe_pr_m_pcg')] + \
        [('nos7', 'pipe_pr_cg', 'rand', 400), ('nos7', 'pipe_pr_m_cg', 'ones', 800)]


def case_id(c):
    return '-'.join(str(q) for q in c)


@pytest.fixture(scope='module')
def amd():
    from new_cg_variants_amd import _lib, device, problems
    return dict(L=_lib, device=device, problems=problems)


@pytest.fixture(scope='module')
def problem(amd, matrices):
    """(operator, right-hand side) -> (A, b, inverse diagonal), built once per module and left unchanged"""
    P = amd['problems']
    make = {'s3_small': lambda: P.WORKLOADS['s3_small']['make'](), 's1_small': lambda: P.WORKLOADS['s1_small']['make'](),
            'lap3d': lambda: P.laplace_3d(21, 17, 13), 'fem12': lambda: P.fem_like_3d(12), 'irr10': lambda: P.fem_irregular_3d(10),
            'lap2d_indef': lambda: P.laplace_2d(64, 48) - 0.02 * sp.identity(64 * 48),
            'lap27_indef': lambda: P.laplace_2d(27, 27) - 0.05 * sp.identity(27 * 27)}
    mats, cache = {}, {}

    def get(operator, rhs='ref'):
        if operator not in mats:
            mats[operator] = sp.csr_matrix(make[operator]()) if operator in make else matrices[operator][0]
        A = mats[operator]
        n = A.shape[0]
        if (operator, rhs) not in cache:
            if rhs == 'ref':
                b = P.reference_rhs(A, n)[0] if operator in make else np.asarray(matrices[operator][1]['b'], dtype=np.float64)
            else:
                b = {'ones': np.ones(n), 'rand': np.random.default_rng(7).standard_normal(n), 'zero': np.zeros(n)}[rhs]
            cache[(operator, rhs)] = (A, b, 1 / A.diagonal())
        return cache[(operator, rhs)]
    return get


def open_operator(amd, A, operator):
    return amd['device'].DeviceCSR(A, knobs=dict(OPERATORS[operator][0]))


def check_family(A, operator, jac, rec):
    """the schedule the case is there for, from the flags and tables the session reports; returns the oracle's dot of the
    iteration launches (the start-up inner products of every pipelined single session: launch_pipe_dots, device_dot)"""
    s, lay = rec['schedule'], rec['layout']
    family = OPERATORS[operator][1]
    if family == 'small' and jac:
        family = 'window'
    assert s['fused'] and not s['comm'] and not s['fused_comm'], s
    assert s['small'] == (family == 'small'), s
    if family == 'small':
        return wg_dot
    assert lay['grid'] > 0, lay['grid']
    assert s['window'] == (family == 'window') and lay['window'] == s['window'], s
    assert s['sliced_rows'] == (family in ('sell', 'sell_win')) and lay['sliced'] == s['sliced_rows'], s
    if family == 'window':
        return OneLaunchTree(lay).dot
    if s['sliced_rows']:
        assert s['window_codes'] == (family == 'sell_win'), s                 # k_sell_win / k_sell_tiles
    else:
        assert np.diff(A.indptr).max() <= tile_cap_nnz(s['tile_steps'])       # no long rows: SciPy's product is the device's
    return UnitTree.of(lay).dot


def same_launch(a, b):
    return a['layout']['grid'] == b['layout']['grid'] and a['layout']['waves_per_block'] == b['layout']['waves_per_block']


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_header_and_binding():
    from new_cg_variants_amd import _lib as L
    text = open(os.path.join(ROOT, 'include', 'prcg.h')).read()
    pub = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = L.lib()
    for name in ('prcg_set_stop', 'prcg_get_stop'):
        assert re.search(rf'\bint\s+{name}\s*\(\s*prcg_t\s*\*', pub), name
        assert name in L._SIGNATURES and hasattr(lib, name), name
    assert lib.prcg_version() == 1
    section = text[text.index('a single PIPELINED session stopped at a residual threshold'):text.index('a BATCH of small independent systems')]
    for word in ('prcg_set_stop', 'prcg_get_stop', 'rr <= *rr_stop', 'breakdown', 'converged', 'NULL clears', 'PRCG_FUSED=0', 'replace hook',
                 'stored-tilde', 'prcg_set_vector, prcg_set_scalars and prcg_set_iteration'):
        assert word in section, word


def test_python_argument_checks_come_before_any_device_call(monkeypatch, matrices):
    import inspect

    import new_cg_variants_amd.callbacks as cbs
    import new_cg_variants_amd.cg_variants as cgv
    from new_cg_variants_amd import device

    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(cgv, 'DeviceCSR', no_device)
    monkeypatch.setattr(cgv, '_operator', no_device)
    A, z = matrices['bcsstk03']
    b = np.asarray(z['b'], dtype=np.float64)
    n = A.shape[0]
    x0 = np.zeros(n)
    for name in PIPELINED:
        f = getattr(cgv, name)
        for key in ('rtol', 'atol'):
            with pytest.raises(ValueError, match=rf'{name}: {key} must be one value or 1 values, one per system -- got shape \(2,\)'):
                f(A, b, x0, 5, **{key: [1e-8, 1e-8]})
            with pytest.raises(ValueError, match=rf'{name}: {key}\[0\] = nan: the value of system 0 must be finite and >= 0'):
                f(A, b, x0, 5, **{key: np.nan})
            with pytest.raises(ValueError, match=rf'{name}: {key}\[0\] = inf'):
                f(A, b, x0, 5, **{key: np.inf})
            with pytest.raises(ValueError, match=rf'{name}: {key}\[0\] = -1.0'):
                f(A, b, x0, 5, **{key: -1.0})
        with pytest.raises(ValueError, match=rf'{name}: b must have shape \({n},\)'):
            f(A, b[:-1], x0, 5, rtol=1e-8)
        # what IS served gets as far as the device: either keyword, both, zero, a Jacobi object or lambda
        for kw in (dict(rtol=1e-8), dict(atol=[1e-3]), dict(rtol=1e-8, atol=1e-12), dict(rtol=0.0)):
            with pytest.raises(AssertionError, match='the device was reached'):
                f(A, b, x0, 5, callbacks=[cbs.updated_residual_2_norm], **kw)
        if name.endswith('_pcg'):
            d = 1 / A.diagonal()
            for prec in (cgv.Jacobi(A), lambda v: d * v):
                with pytest.raises(AssertionError, match='the device was reached'):
                    f(A, b, x0, 5, preconditioner=prec, rtol=1e-8)
            # a preconditioner that is no diagonal scaling runs the stored-tilde schedule: refused here, not on the device
            for prec in (cgv.BlockJacobi(A, 2), lambda v: np.roll(v, 1)):
                with pytest.raises(ValueError, match=rf'{name}: rtol= / atol= serve no preconditioner but a diagonal scaling.*stored-tilde schedule'):
                    f(A, b, x0, 5, preconditioner=prec, rtol=1e-8)
            with pytest.raises(AssertionError, match='the device was reached'):       # ... and is served without the keywords, as ever
                f(A, b, x0, 5, preconditioner=cgv.BlockJacobi(A, 2))
    # the functions that cannot stop never took the keywords and pass them by like any keyword they do not know: unchanged
    for name in ('hs_cg', 'pr_pcg', 'cg_cg', 'gv_pcg'):
        with pytest.raises(AssertionError, match='the device was reached'):
            getattr(cgv, name)(A, b, x0, 5, rtol=-1.0)
    assert inspect.signature(device.DeviceCSR.begin).parameters['rr_stop'].default is None
    assert callable(device.DeviceCSR.stop)
    # the batch's thresholds and the single functions' come from one place
    thr = cgv._stop_thresholds('f', 1e-3, 1e-9, [b, 2 * b])
    assert np.array_equal(thr, np.maximum(1e-3 * np.array([np.linalg.norm(b), np.linalg.norm(2 * b)]), 1e-9) ** 2)
    assert cgv._stop_thresholds('f', None, None, [b]) is None


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('operator,method,rhs,max_iter', CASES, ids=[case_id(c) for c in CASES])
def test_a_session_stops_where_the_oracle_does(amd, problem, operator, method, rhs, max_iter):
    """Five sessions on one handle.  (0) without a threshold, one prcg_iterate call: its layout gives the oracle's tree, the
    oracle gives thr = rr at max_iter // 2 and the stop.  (1) rr_stop = thr, one prcg_iterate(max_iter - 1) call: the stop is
    decided by the prologue of launch k_stop + 1 (one-workgroup solver: inside its loop).  (2a) calls of k_stop and the rest: the
    final reduction of the first call decides; (2b) calls of k_stop + 1 and the rest: the prologue of that call's last launch.
    No synchronisation between the calls: the later launches find the session stopped.  (3) a further prcg_iterate(3) after
    (1) changes nothing.  All three hold the oracle's state at k_stop bit for bit: stop word, x r p s w u (r~ s~; w~), scalar
    rows 0..k_stop, coefficient rows 1..k_stop, the history; everything beyond reads zero; prcg_iteration is k_stop.  (4) thr = 0:
    never stops, and every vector, scalar, coefficient and history entry equals session (0) -- which differs in schedule only
    by the deferred (x,p) store, where that exists."""
    L = amd['L']
    _, _, jac = METHODS[method]
    A, b, inv_diag = problem(operator, rhs)
    d = inv_diag if jac else None
    op = open_operator(amd, A, operator)
    try:
        free = run_session(L, op, method, b, d, max_iter, None, (max_iter - 1,))
        dot = check_family(A, operator, jac, free)
        traj = trajectory(A, b, method, dot, device_dot, max_iter - 1, keep=())
        thr = float(traj['scalars'][max_iter // 2, 4])
        k_stop, status = stop_of(traj, thr)
        print(f'{case_id((operator, method, rhs, max_iter))}: thr = {thr!r}, the oracle stops at k = {k_stop} with status {status}; '
              f'{free["layout"]["grid"]} workgroups x {free["layout"]["waves_per_block"]} waves')
        assert np.isfinite(thr) and thr > 0 and 0 < k_stop < max_iter - 1 and status in (CONVERGED, BREAKDOWN), (thr, k_stop, status)
        assert np.isfinite(traj['scalars'][:k_stop + 1]).all() and np.isfinite(traj['coef'][:k_stop]).all()
        assert stop_of(traj, 0.0) == (-1, 0), 'the run breaks down: a wrong case for the thr = 0 comparison'
        traj = trajectory(A, b, method, dot, device_dot, max_iter - 1, keep=(k_stop, max_iter - 1))
        assert all(np.isfinite(v).all() for v in traj['at'][k_stop].values())
        assert free['schedule']['xp_deferred'] == (free['schedule']['window'] and not free['schedule']['small'])
        holds_trajectory(free, traj, max_iter - 1, 0, max_iter, 'no threshold')
        rest = max_iter - 1 - k_stop
        one = run_session(L, op, method, b, d, max_iter, thr, (max_iter - 1,), then=3)
        at_end = run_session(L, op, method, b, d, max_iter, thr, (k_stop, rest))
        past = run_session(L, op, method, b, d, max_iter, thr, (k_stop + 1, rest - 1))
        never = run_session(L, op, method, b, d, max_iter, 0.0, (max_iter - 1,))
    finally:
        op.close()
    for what, rec in (('one call', one), ('a call ends at k_stop', at_end), ('a call ends at k_stop + 1', past)):
        assert not rec['schedule']['xp_deferred'] and same_launch(rec, free), (what, rec['schedule'])
        assert rec['schedule']['small'] == free['schedule']['small'] and rec['schedule']['fused']
        holds_trajectory(rec, traj, k_stop, status, max_iter, what)
    assert same_reading(one, one['again']), 'prcg_iterate on a stopped session is a no-op'
    assert not never['schedule']['xp_deferred'] and same_launch(never, free)
    assert never['stop'] == (-1, 0) and never['k'] == max_iter - 1
    assert same_reading(never, free), 'thr = 0 on a run that does not stop: the bits of the session without a threshold'


@pytest.mark.gpu
@pytest.mark.parametrize('operator,method', [('s3_small', 'pipe_pr_cg'), ('fem12', 'pipe_pr_m_pcg'), ('bcsstk14', 'pipe_p_pcg'), ('nos7', 'pipe_pr_cg')])
def test_a_zero_right_hand_side_stops_before_the_first_iteration(amd, problem, operator, method):
    """b = 0, x0 = 0, thr = 0: rr = 0 <= 0 on row 0 -- stopped at 0, converged, whatever mu is; no row beyond 0 is written"""
    L = amd['L']
    A, b, inv_diag = problem(operator, 'zero')
    max_iter = 9
    op = open_operator(amd, A, operator)
    try:
        rec = run_session(L, op, method, b, inv_diag if METHODS[method][2] else None, max_iter, 0.0, (3, 5), then=2)
    finally:
        op.close()
    assert rec['stop'] == (0, CONVERGED) and rec['k'] == 0
    assert all(np.array_equal(v, np.zeros(A.shape[0])) for v in rec['at'].values())
    assert np.array_equal(rec['scalars'], np.zeros((max_iter, 8))) and np.array_equal(rec['coef'], np.zeros((max_iter - 1, 3)))
    assert np.array_equal(rec['hist'], np.zeros(max_iter))
    assert same_reading(rec, rec['again'])


@pytest.mark.gpu
@pytest.mark.parametrize('operator,method,max_iter', [('lap27_indef', 'pipe_pr_cg', 30), ('lap2d_indef', 'pipe_pr_cg', 30), ('lap2d_indef', 'pipe_pr_pcg', 30),
                                                      ('lap2d_indef', 'pipe_p_cg', 30)])
def test_a_breakdown_stops_the_session(amd, problem, operator, method, max_iter):
    """A symmetric INDEFINITE operator (a shifted 5-point Laplacian) and a threshold far below what the run reaches: mu = p.s turns
    negative at an interior k and the rule stops the session there with status 2 -- on the one-workgroup solver (lap27_indef,
    n = 729: module docstring for why not nos7) and on the one-launch schedule (lap2d_indef, n = 3072, with and without Jacobi).
    The oracle's status is asserted first; x at the stop is finite."""
    L = amd['L']
    _, _, jac = METHODS[method]
    A, b, inv_diag = problem(operator)
    d = inv_diag if jac else None
    thr = 1e-300
    op = open_operator(amd, A, operator)
    try:
        free = run_session(L, op, method, b, d, max_iter, None, (max_iter - 1,))       # (runs into inf / nan: nobody stops it)
        dot = check_family(A, operator, jac, free)
        traj = trajectory(A, b, method, dot, device_dot, max_iter - 1)
        k_stop, status = stop_of(traj, thr)
        print(f'{operator} {method}: the oracle breaks down at k = {k_stop}: mu, nu, rr = {traj["scalars"][k_stop, [0, 3, 4]]}')
        assert status == BREAKDOWN and 0 < k_stop < max_iter - 1, (k_stop, status)
        assert np.isfinite(traj['scalars'][:k_stop + 1]).all() and np.isfinite(traj['at'][k_stop]['x']).all()
        one = run_session(L, op, method, b, d, max_iter, thr, (max_iter - 1,), then=3)
        at_end = run_session(L, op, method, b, d, max_iter, thr, (k_stop, max_iter - 1 - k_stop))
    finally:
        op.close()
    for what, rec in (('one call', one), ('a call ends at k_stop', at_end)):
        holds_trajectory(rec, traj, k_stop, BREAKDOWN, max_iter, what)
        assert np.isfinite(rec['at']['x']).all()
    assert same_reading(one, one['again'])


@pytest.mark.gpu
def test_what_a_threshold_does_not_serve_is_refused(amd, problem):
    """through the C-ABI, each with its message; nothing falls back to a schedule that cannot stop"""
    L = amd['L']
    lib = L.lib()
    A, b, inv_diag = problem('s1_small')
    n = A.shape[0]
    x0 = np.zeros(n)
    op = open_operator(amd, A, 's1_small')
    h = op._h
    k_stop, status = np.full(1, 7, dtype=np.int32), np.full(1, 7, dtype=np.int32)

    def error():
        return lib.prcg_last_error(h).decode()

    def begin(variant, d=None):
        return lib.prcg_solve_begin(h, variant, L.ptr(b), L.ptr(x0), 12, None, L.ptr(d), 1)
    try:
        assert lib.prcg_get_stop(h, L.ptr(k_stop), L.ptr(status)) == L.EINVAL and 'prcg_get_stop: no open session' in error()
        assert k_stop[0] == status[0] == 7
        good = np.array([1e-30])
        assert lib.prcg_set_stop(h, L.ptr(good)) == L.OK
        for bad, text in ((np.nan, 'nan'), (np.inf, 'inf'), (-np.inf, '-inf'), (-1e-300, '-1e-300')):
            assert lib.prcg_set_stop(h, L.ptr(np.array([bad]))) == L.EINVAL
            assert re.search(rf'prcg_set_stop: rr_stop = {re.escape(text)}: the threshold must be finite and >= 0', error()), error()
        served = 'which serves the pipelined variants'
        for variant in (L.HS, L.PR, L.M, L.CG_CG, L.GV):
            assert begin(variant) == L.EINVAL
            assert served in error() and f'variant {variant} is not pipelined' in error(), error()
        assert lib.prcg_get_stop(h, L.ptr(k_stop), L.ptr(status)) == L.EINVAL          # (a refused begin opens nothing)
        op.build_block_jacobi(2)
        assert begin(L.PIPE_PR) == L.EINVAL and served in error() and 'host-callback or block-Jacobi preconditioner is in force' in error(), error()
        assert begin(L.PIPE_PR, inv_diag) == L.OK          # (inv_diag overrides the blocks: the diagonal scaling is served)
        op.set_block_jacobi(0, None)
        fn = L.PREC_FN(lambda ctx, count, v, out: 1)
        import ctypes as C
        assert lib.prcg_set_preconditioner(h, C.cast(fn, C.c_void_p), None) == L.OK
        assert begin(L.PIPE_PR_M) == L.EINVAL and 'host-callback or block-Jacobi preconditioner is in force' in error(), error()
        assert lib.prcg_set_preconditioner(h, None, None) == L.OK
        hook = L.REPLACE_FN(lambda ctx, k: 0)
        assert lib.prcg_set_replace_hook(h, C.cast(hook, C.c_void_p), None) == L.OK
        assert begin(L.PIPE_P) == L.EINVAL and served in error() and 'a replace hook is set' in error(), error()
        assert lib.prcg_set_replace_hook(h, None, None) == L.OK
        # a session begun with a threshold: running -> {-1, 0}; its state is not set from outside
        assert begin(L.PIPE_P_M) == L.OK
        assert lib.prcg_get_stop(h, L.ptr(k_stop), L.ptr(status)) == L.OK and (k_stop[0], status[0]) == (-1, 0)
        assert lib.prcg_get_stop(h, None, L.ptr(status)) == L.EINVAL and 'null buffer' in error()
        row = np.zeros(8)
        for rc, name in ((lib.prcg_set_vector(h, L.VEC['x'], L.ptr(x0)), 'prcg_set_vector'), (lib.prcg_set_scalars(h, 0, L.ptr(row)), 'prcg_set_scalars'),
                         (lib.prcg_set_iteration(h, 0), 'prcg_set_iteration')):
            assert rc == L.EINVAL, name
        assert 'prcg_set_iteration: the open session was begun with a stop threshold' in error(), error()
        assert lib.prcg_set_vector(h, L.VEC['x'], L.ptr(x0)) == L.EINVAL and 'prcg_set_vector: the open session was begun with a stop threshold' in error()
        # cleared: everything is served again, a session has no stop, the setters work
        assert lib.prcg_set_stop(h, None) == L.OK
        assert begin(L.HS) == L.OK
        assert lib.prcg_get_stop(h, L.ptr(k_stop), L.ptr(status)) == L.OK and (k_stop[0], status[0]) == (-1, 0)
        assert lib.prcg_set_vector(h, L.VEC['x'], L.ptr(x0)) == L.OK
    finally:
        op.close()
    # PRCG_FUSED=0 selects the two-kernel schedule, which cannot stop
    op = amd['device'].DeviceCSR(A, knobs={'PRCG_FUSED': '0'})
    try:
        with pytest.raises(L.PrcgError, match='PRCG_FUSED=0 selects the two-kernel schedule, which cannot stop'):
            op.begin(L.PIPE_PR, b, x0, 12, rr_stop=1.0)
        op.begin(L.PIPE_PR, b, x0, 12)
        assert op.stop() == (-1, 0)
    finally:
        op.close()


@pytest.mark.gpu
def test_cg_variants_stop_at_rtol(amd, problem):
    """pipe_pr_pcg(..., preconditioner=Jacobi(A), rtol=1e-8) on fem_like_3d(12): 'iterations', 'status' and the history are those
    of a session begun with rr_stop = (rtol ||b||)^2 in one call, which are the oracle's; a foreign callback is called k_stop + 1
    times -- for k = 0 .. k_stop, on the states of the run -- and never after the stop"""
    import new_cg_variants_amd.callbacks as cbs
    import new_cg_variants_amd.cg_variants as cgv
    L = amd['L']
    A, b, inv_diag = problem('fem12')
    n, max_iter, rtol = A.shape[0], 120, 1e-8
    thr = float(np.maximum(rtol * np.linalg.norm(b), 0.0) ** 2)
    op = open_operator(amd, A, 'fem12')
    try:
        rec = run_session(L, op, 'pipe_pr_pcg', b, inv_diag, max_iter, thr, (max_iter - 1,))
        dot = check_family(A, 'fem12', True, rec)
    finally:
        op.close()
    traj = trajectory(A, b, 'pipe_pr_pcg', dot, device_dot, max_iter - 1, keep=())
    k_stop, status = stop_of(traj, thr)
    print(f'fem12 pipe_pr_pcg rtol = {rtol}: thr = {thr!r}, the oracle stops at k = {k_stop} with status {status}')
    assert 0 < k_stop < max_iter - 1 and status in (CONVERGED, BREAKDOWN)
    assert rec['stop'] == (k_stop, status) and rec['k'] == k_stop
    assert np.array_equal(rec['hist'][:k_stop + 1], np.sqrt(traj['scalars'][:k_stop + 1, 4])) and not rec['hist'][k_stop + 1:].any()
    cgv.clear_operator_cache()
    try:
        out = cgv.pipe_pr_pcg(A, b, np.zeros(n), max_iter, preconditioner=cgv.Jacobi(A), rtol=rtol, callbacks=[cbs.updated_residual_2_norm])
        assert out['iterations'] == k_stop and out['status'] == ('converged' if status == CONVERGED else 'breakdown')
        assert np.array_equal(out['updated_residual_2_norm'], rec['hist'])
        seen = []

        def foreign(**env):
            seen.append((env['k'], float(env['nu_k']), env['x_k'].copy()))
        out2 = cgv.pipe_pr_pcg(A, b, np.zeros(n), max_iter, preconditioner=cgv.Jacobi(A), rtol=rtol, callbacks=[cbs.updated_residual_2_norm, foreign])
        assert [k for k, _, _ in seen] == list(range(k_stop + 1)), [k for k, _, _ in seen]
        assert [nu for _, nu, _ in seen] == traj['scalars'][:k_stop + 1, 3].tolist()
        assert out2['iterations'] == k_stop and out2['status'] == out['status']
        assert np.array_equal(out2['updated_residual_2_norm'], rec['hist'])
        assert np.array_equal(seen[-1][2], rec['at']['x'])
        # without the keywords: no stop, no new keys -- the function as it was
        out3 = cgv.pipe_pr_pcg(A, b, np.zeros(n), 12, preconditioner=cgv.Jacobi(A), callbacks=[cbs.updated_residual_2_norm])
        assert 'iterations' not in out3 and 'status' not in out3 and (out3['updated_residual_2_norm'] > 0).all()
        # atol alone, far above the initial residual: stopped at 0
        out4 = cgv.pipe_pr_cg(A, b, np.zeros(n), 12, atol=1e3 * np.linalg.norm(b), callbacks=[cbs.updated_residual_2_norm])
        assert out4['iterations'] == 0 and out4['status'] == 'converged' and not out4['updated_residual_2_norm'][1:].any()
        # a run that ends before the threshold is reached
        out5 = cgv.pipe_pr_m_cg(A, b, np.zeros(n), 6, rtol=1e-30, callbacks=[cbs.updated_residual_2_norm])
        assert out5['iterations'] == 5 and out5['status'] == 'max_iter' and (out5['updated_residual_2_norm'] > 0).all()
    finally:
        cgv.clear_operator_cache()
