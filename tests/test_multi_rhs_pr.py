"""Two right-hand sides in one predict-and-recompute session (prcg.h: prcg_solve_begin_multi with PRCG_PR / PRCG_M;
DeviceCSR.begin_multi; cg_variants.pr_cg_multi / pr_pcg_multi / m_cg_multi / m_pcg_multi).

The session runs, per column, exactly the recurrence of pr_pcg / m_pcg (pr_cg.py:93-176; without Jacobi the identity-
preconditioned one), and every inner product is summed in the order tests/device_order.py: device_sum models.  So the
oracle (oracle/ne_oracle.py) run with ``dot=device_dot`` and ``square=lambda a: a*a`` (the device multiplies) is asked
for EQUAL BITS: vectors, the five inner products of every iteration, alpha, beta, the predicted nu, the history.  No
tolerance anywhere.

The recorded history is compared with sqrt(device_dot(r_k, r_k)) of the oracle's r_k, as in tests/test_multi_rhs.py.
The oracle runs are computed once per (operator, variant, preconditioner, right-hand side) and shared; nobody writes
to them.  The harness shared with the other multi-RHS files: tests/multi_rhs_common.py.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

import multi_rhs_common as common
from device_order import chunking
from multi_rhs_common import KNOBS, VECS, _raises, amd, assert_column_bits, assert_finite, operator, same, single_session      # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_column(A, b, x0, iters, jacobi, variant='pr'):
    """pr_pcg / m_pcg of the oracle with the device's summation order and its a * a: the state after `iters` iterations,
    mu, delta, gamma, nu, rr of every iteration, the coefficients used BY every iteration >= 1, the recorded history."""
    return common.pr_column(A, b, x0, iters, jacobi, variant)


def device_columns(op, L, variant, B, X0, iters, inv_diag, chunks=(1, 2, 7)):
    """A two-RHS session of `variant` on `op`, read through the per-column getters: per column the vectors, ALL scalar slots
    of every iteration, the three coefficients of every iteration >= 1 and the history; and the schedule."""
    def begin():
        op.begin_multi(variant, B, X0, iters + 1, inv_diag=inv_diag, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM)
    tilde = () if inv_diag is None else ('rt',) if variant == L.HS else ('rt', 'st')
    return common.device_columns(op, L, begin, iters, 2, VECS + tilde, common.served_slots(L, variant == L.HS), chunks,
                                 report=common.served_slots(L, False))


def problem(name, x0_nonzero=False):
    """(A, B, X0) of an operator: the right-hand sides of tests/multi_rhs_common.py: two_rhs"""
    return common.problem(name, 2, x0_nonzero)


# reference(name, variant, jacobi, iters, x0_nonzero, column): the oracle run of one column, computed once and shared (read-only).
# column: 0, 1, or 'zero' (b = 0)
reference = functools.partial(common.reference, oracle_column, 2)


# K per case: 60 where nothing else decides.  s3_small with Jacobi: the oracle's nu reaches <= 0 at iteration 6 (Meurant's
# prediction) and 8 (pr) on that diagonally dominant band, so 5 there.  Every case asserts its oracle run finite, mu, nu > 0.
def _iters(name, jacobi):
    return 5 if (name, jacobi) == ('s3_small', True) else 60


CASES = ([('pr', name, jac, _iters(name, jac), False)
          for name in ('s3_small', 's1_small', 'lap3d', 'fem12', 'fem_irregular10', 'bcsstk14', 'bcsstk14_csr')
          for jac in (False, True)]
         + [('m', name, jac, _iters(name, jac), False) for name in ('s3_small', 'fem12', 'bcsstk14') for jac in (False, True)]
         + [('pr', 'fem12', True, 60, True)])


@pytest.mark.gpu
@pytest.mark.parametrize('variant,name,jacobi,iters,x0_nonzero', CASES)
def test_bits_against_the_device_ordered_oracle(amd, variant, name, jacobi, iters, x0_nonzero):
    """Both columns of a PR / M two-RHS session against two oracle runs: x, r, p, s, (rt, st), mu / delta / gamma / nu / rr
    of every iteration, alpha, beta, the predicted nu and the history -- equal bits."""
    L = amd['L']
    matrix = 'bcsstk14' if name == 'bcsstk14_csr' else name          # the same matrix, another product family: one oracle run
    A, B, X0 = problem(matrix, x0_nonzero)
    _, family = operator(name)
    n = A.shape[0]
    want = [reference(matrix, variant, jacobi, iters, x0_nonzero, j) for j in range(2)]
    for j in range(2):
        assert_finite(want[j], f'{variant} {name} jacobi={jacobi} column {j}')
    inv_diag = 1 / A.diagonal() if jacobi else None
    op = amd['device'].DeviceCSR(A, knobs=KNOBS.get(name))
    try:
        got, sched = device_columns(op, L, {'pr': L.PR, 'm': L.M}[variant], B, X0, iters, inv_diag)
    finally:
        op.close()
    assert sched['rhs2'] and not sched['small'] and not sched['fused'], sched
    for key, val in family.items():
        assert sched[key] == val, (name, key, sched)
    for j in range(2):
        assert_column_bits(got[j], want[j], f'{variant} {name} jacobi={jacobi} column {j}')
    print(f'{variant} {name} jacobi={jacobi}: n={n}, {iters} iterations, both columns bit-exact; schedule {sched}')


@pytest.mark.gpu
def test_two_trips_per_block(amd):
    """laplace_3d(102, 102, 101): n = 1,050,804 > 2048 * 512, chunking(n) = (1027, 2) -- the smallest shape at which the vector
    kernels' trip loop, their `base >= n` exit and their ragged last block run.  pr with Jacobi, 3 iterations in chunks (2, 1)."""
    L = amd['L']
    A, B, X0 = problem('lap3d_two_trips')
    n = A.shape[0]
    assert n == 1050804 and chunking(n) == (1027, 2)
    iters = 3
    want = [reference('lap3d_two_trips', 'pr', True, iters, False, j) for j in range(2)]
    for j in range(2):
        assert_finite(want[j], f'two trips, column {j}')
    op = amd['device'].DeviceCSR(A)
    try:
        got, sched = device_columns(op, L, L.PR, B, X0, iters, 1 / A.diagonal(), chunks=(2, 1))
    finally:
        op.close()
    assert sched['rhs2'] and not sched['small'] and not sched['fused'], sched
    for j in range(2):
        assert_column_bits(got[j], want[j], f'two trips, column {j}', keys=('x', 'r', 'scalars', 'alpha', 'beta', 'nu_pred'))


@pytest.mark.gpu
@pytest.mark.parametrize('jacobi', [False, True])
def test_columns_are_independent(amd, jacobi):
    """Swapped right-hand sides give swapped bits, equal ones equal columns, and a column that breaks down at once
    (b = 0, x0 = 0: 0 / 0) leaves the other column's bits alone while its own history holds the NaNs."""
    L = amd['L']
    A, B, X0 = problem('fem12')
    n = A.shape[0]
    inv_diag = 1 / A.diagonal() if jacobi else None
    iters = 25
    op = amd['device'].DeviceCSR(A)
    try:
        ab, _ = device_columns(op, L, L.PR, B, X0, iters, inv_diag)
        ba, _ = device_columns(op, L, L.PR, B[::-1], X0, iters, inv_diag)
        aa, _ = device_columns(op, L, L.PR, np.stack([B[0], B[0]]), X0, iters, inv_diag)
        a0, _ = device_columns(op, L, L.PR, np.stack([B[0], np.zeros(n)]), X0, iters, inv_diag)
    finally:
        op.close()
    assert_column_bits(ba[1], ab[0], 'swapped: column 1 of (b1, b0) vs column 0 of (b0, b1)')
    assert_column_bits(ba[0], ab[1], 'swapped: column 0 of (b1, b0) vs column 1 of (b0, b1)')
    assert_column_bits(aa[1], aa[0], '(b0, b0): the two columns')
    assert_column_bits(aa[0], ab[0], '(b0, b0) vs (b0, b1): column 0')
    assert_column_bits(a0[0], aa[0], '(b0, 0): column 0 beside a column that broke down')
    assert np.isfinite(a0[0]['hist']).all()
    assert_column_bits(ab[0], reference('fem12', 'pr', jacobi, iters, False, 0), 'column 0 vs the oracle')
    want = reference('fem12', 'pr', jacobi, iters, False, 'zero')
    assert want['hist'][0] == 0.0 and np.isnan(want['hist'][1:]).all()
    assert_column_bits(a0[1], want, '(b0, 0): the column that broke down')


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['fem12', 's3_small'])
def test_nothing_else_moved(amd, name):
    """On ONE handle: a single pr session, an HS two-RHS session, a PR two-RHS session, the HS two-RHS session again, the
    single pr session again.  The single runs are bitwise equal and equal to a fresh handle's; the HS two-RHS runs are
    bitwise equal in every vector, scalar slot, coefficient and history, their out[2] is 0 and only mu, nu, rr are set."""
    L = amd['L']
    A, B, X0 = problem(name)
    n = A.shape[0]
    iters, multi_iters = 24, 5
    d = 1 / A.diagonal()
    op = amd['device'].DeviceCSR(A)
    fresh = amd['device'].DeviceCSR(A)
    try:
        first = single_session(op, L, L.PR, B[0], np.zeros(n), iters)
        hs_a, sched_a = device_columns(op, L, L.HS, B, X0, multi_iters, d)
        pr2, sched_pr = device_columns(op, L, L.PR, B, X0, multi_iters, d)
        hs_b, sched_b = device_columns(op, L, L.HS, B, X0, multi_iters, d)
        again = single_session(op, L, L.PR, B[0], np.zeros(n), iters)
        other = single_session(fresh, L, L.PR, B[0], np.zeros(n), iters)
    finally:
        op.close()
        fresh.close()
    assert sched_a['rhs2'] and sched_pr['rhs2'] and sched_b == sched_a
    assert not first[0]['rhs2'] and not again[0]['rhs2']
    for run, what in ((again, 'after the two-RHS sessions'), (other, 'fresh handle')):
        assert run[0] == first[0], (what, run[0], first[0])
        for v_ in VECS:
            assert same(run[1][v_], first[1][v_]), (what, v_)
        assert same(run[2], first[2]) and same(run[3], first[3]) and same(run[4], first[4]), what
    for j in range(2):
        for q in VECS + ('rt', 'all_scalars', 'alpha', 'beta', 'nu_pred', 'hist'):
            assert same(hs_a[j][q], hs_b[j][q]), (j, q)
        assert hs_a[j]['st'] is None
        assert not hs_a[j]['nu_pred'].any(), 'Hestenes-Stiefel predicts no nu: out[2] stays 0'
        assert not hs_a[j]['all_scalars'][:, [L.S_DELTA, L.S_GAMMA, L.S_RES2, L.S_ERRA2, L.S_ERR2]].any()
        assert_column_bits(pr2[j], reference(name, 'pr', True, multi_iters, False, j), f'{name}: the PR session in between, column {j}')


@pytest.mark.gpu
def test_refusals(amd):
    """What the two-RHS session does not serve stays PRCG_EINVAL with a text naming the reason, for PRCG_PR / PRCG_M as for
    PRCG_HS; inside a PR two-RHS session the single-column accessors are refused."""
    L, cgv = amd['L'], amd['cgv']
    A, B, X0 = problem('fem12')
    n = A.shape[0]
    d = 1 / A.diagonal()
    lib = L.lib()
    op = amd['device'].DeviceCSR(A)
    try:
        for v in (L.PIPE_PR, L.CG_CG, L.GV):
            with _raises(L, r'PRCG_HS \(hs_cg / hs_pcg\), PRCG_PR \(pr_cg / pr_pcg\) and PRCG_M \(m_cg / m_pcg\) only'):
                op.begin_multi(v, B, X0, 8)
        with _raises(L, 'history bits other than PRCG_HIST_UPDATED_RESIDUAL_2_NORM'):
            op.begin_multi(L.PR, B, X0, 8, hist_mask=L.HIST_RESIDUAL_2_NORM)
        three = (C.c_void_p * 3)(B[0].ctypes.data, B[1].ctypes.data, B[0].ctypes.data)
        rc = lib.prcg_solve_begin_multi(op._h, L.PR, 3, three, three, 8, None, 0)
        assert rc == L.EINVAL and b'nrhs = 3' in lib.prcg_last_error(op._h)
        # a host-callback preconditioner left on the handle
        op.begin(L.PR, B[0], X0[0], 4, preconditioner=lambda v: 0.5 * v[::-1][::-1] + 0.0)
        with _raises(L, 'host-callback preconditioner'):
            op.begin_multi(L.PR, B, X0, 8)
        # block Jacobi left on the handle
        bj = cgv.BlockJacobi(A, 3)
        op.begin(L.PR, B[0], X0[0], 4, block_jacobi=(3, bj.inv_blocks))
        with _raises(L, 'block-Jacobi preconditioner'):
            op.begin_multi(L.M, B, X0, 8)
        op.clear_preconditioners()
        op.set_replace_hook(lambda k: False)
        with _raises(L, 'replace hook'):
            op.begin_multi(L.PR, B, X0, 8)
        op.set_replace_hook(None)
        # inside a PR two-RHS session without Jacobi
        op.begin_multi(L.PR, B, X0, 8, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM)
        op.iterate(2)
        for call in (lambda: op.get_vector('x'), lambda: op.set_vector('x', B[0]), lambda: op.get_scalars(1),
                     lambda: op.set_scalars(1, np.zeros(L.NUM_SCALARS)), lambda: op.get_coefficients(1),
                     lambda: op.history(), lambda: op.set_iteration(1)):
            with _raises(L, 'two right-hand sides'):
                call()
        with _raises(L, 'right-hand side 2 out of range'):
            op.get_vector('x', rhs=2)
        for name in ('rt', 'st', 'w'):
            with _raises(L, 'not part of the two-RHS session'):
                op.get_vector(name, rhs=0)
        op.iterate(1)                            # the session is intact after the refusals
        op.sync()
        assert op.k == 3 and np.isfinite(op.get_vector('x', rhs=1)).all()
        # ... and with Jacobi: rt and st are answered, w is not
        op.begin_multi(L.PR, B, X0, 8, inv_diag=d)
        op.iterate(2)
        rt, st = op.get_vector('rt', rhs=0), op.get_vector('st', rhs=0)
        assert same(st, d * op.get_vector('s', rhs=0)) and np.isfinite(rt).all() and rt.any()
        with _raises(L, 'not part of the two-RHS session'):
            op.get_vector('w', rhs=0)
        op.iterate(1)
        op.sync()
        assert op.k == 3 and np.isfinite(op.get_vector('x', rhs=1)).all()
    finally:
        op.close()
    # ghost columns
    ghost = amd['device'].DeviceCSR(sp.hstack([A, sp.csr_matrix((n, 5))]).tocsr())
    try:
        with _raises(L, 'n_ghost = 5 > 0'):
            ghost.begin_multi(L.PR, B, X0, 8)
    finally:
        ghost.close()


@pytest.mark.gpu
def test_the_four_functions_return_two_trials(amd):
    """pr_cg_multi / pr_pcg_multi / m_cg_multi / m_pcg_multi: two trial dicts named after the function, the histories those of
    the oracle's columns; Jacobi(A) and a callable that probes as a diagonal are the same session; light host callbacks are
    called per column in (k, j) order."""
    cgv, cbs = amd['cgv'], amd['cbs']
    A, B, X0 = problem('fem12')
    iters = 30
    seen = []

    def light(**env):
        seen.append((env['k'], env['output']['rhs']))
    light.prcg_host_light = True
    rec = [cbs.updated_residual_2_norm]
    d = 1 / A.diagonal()
    try:
        runs = {('pr', False): cgv.pr_cg_multi(A, B, X0, iters + 1, callbacks=rec),
                ('pr', True): cgv.pr_pcg_multi(A, B, X0, iters + 1, preconditioner=cgv.Jacobi(A), callbacks=rec + [light]),
                ('m', False): cgv.m_cg_multi(A, B, X0, iters + 1, callbacks=rec),
                ('m', True): cgv.m_pcg_multi(A, B, X0, iters + 1, preconditioner=cgv.Jacobi(A), callbacks=rec)}
        probed = cgv.pr_pcg_multi(A, B, X0, iters + 1, preconditioner=lambda v: d * v, callbacks=rec)
    finally:
        cgv.clear_operator_cache()
    assert seen == [(k, j) for k in range(iters + 1) for j in range(2)]
    for (variant, jacobi), trials in runs.items():
        name = f'{variant}_{"pcg" if jacobi else "cg"}_multi'
        assert len(trials) == 2
        for j in range(2):
            assert trials[j]['name'] == name and trials[j]['max_iter'] == iters + 1 and trials[j]['rhs'] == j
            want = reference('fem12', variant, jacobi, iters, False, j)
            assert np.isfinite(want['hist']).all()
            assert same(trials[j]['updated_residual_2_norm'], want['hist']), (name, j)
    for j in range(2):
        assert same(probed[j]['updated_residual_2_norm'], runs[('pr', True)][j]['updated_residual_2_norm']), j


# ---- no GPU needed ----------------------------------------------------------------------------------------------------
NAMES = ('pr_cg_multi', 'pr_pcg_multi', 'm_cg_multi', 'm_pcg_multi')


def test_names_and_header():
    """The four functions are public, and the header's two-RHS section names the two new variants and their reference."""
    import new_cg_variants_amd.cg_variants as cgv
    for name in NAMES:
        assert name in cgv.__all__ and callable(getattr(cgv, name)) and getattr(cgv, name).__name__ == name
    text = open(os.path.join(ROOT, 'include', 'prcg.h')).read()
    section = text[text.index('TWO right-hand sides'):text.index('prcg_solve_begin_multi(')]
    for word in ('PRCG_HS', 'PRCG_PR', 'PRCG_M', 'hs_cg.py:9', 'pr_cg.py:166', ':172'):
        assert word in section, word


def test_python_argument_checks_come_before_any_device_call(monkeypatch):
    """The four functions check shapes and refuse what the session does not serve with ValueError -- before an operator is
    uploaded or a library call is made, and without falling back to two sessions."""
    import new_cg_variants_amd.cg_variants as cgv
    import new_cg_variants_amd.callbacks as cbs
    from new_cg_variants_amd import _lib as L, device, problems as P

    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(cgv, '_operator', no_device)
    monkeypatch.setattr(cgv, 'DeviceCSR', no_device)
    A = P.fem_like_3d(4)
    n = A.shape[0]
    B, X0 = np.ones((2, n)), np.zeros((2, n))
    for name in NAMES:
        f = getattr(cgv, name)
        for bad_B, bad_X in ((np.ones(n), X0), (np.ones((3, n)), np.zeros((3, n))), (np.ones((n, 2)), X0), (B, np.zeros(n)),
                             (np.ones((2, n + 1)), X0)):
            with pytest.raises(ValueError, match=r'%s: .* shape \(2, %d\)' % (name, n)):
                f(A, bad_B, bad_X, 5)
        with pytest.raises(ValueError, match='error_A_norm is not served'):
            f(A, B, X0, 5, callbacks=[cbs.error_A_norm])
        with pytest.raises(ValueError, match='needs the state vectors'):
            f(A, B, X0, 5, callbacks=[lambda **env: None])
        with pytest.raises(ValueError, match='x_true'):
            f(A, B, X0, 5, x_true=np.ones(n))
        # what IS served gets as far as the device
        with pytest.raises(AssertionError, match='the device was reached'):
            f(A, B, X0, 5, callbacks=[cbs.updated_residual_2_norm])
    for name in ('pr_pcg_multi', 'm_pcg_multi'):
        f = getattr(cgv, name)
        with pytest.raises(ValueError, match='block-Jacobi'):
            f(A, B, X0, 5, preconditioner=cgv.BlockJacobi(A, 3))
        with pytest.raises(ValueError, match='no diagonal scaling'):
            f(A, B, X0, 5, preconditioner=lambda v: np.roll(v, 1))
        with pytest.raises(AssertionError, match='the device was reached'):
            f(A, B, X0, 5, preconditioner=cgv.Jacobi(A), callbacks=[cbs.updated_residual_2_norm])
    with pytest.raises(ValueError, match='pr_pcg_multi'):
        cgv.pr_cg_multi(A, B, X0, 5, preconditioner=cgv.Jacobi(A))
    with pytest.raises(ValueError, match='m_pcg_multi'):
        cgv.m_cg_multi(A, B, X0, 5, preconditioner=cgv.Jacobi(A))
    # DeviceCSR.begin_multi: shapes are checked before the library is called, whichever variant
    bare = object.__new__(device.DeviceCSR)
    bare.n, bare._lib, bare._h = n, None, None
    for variant in (L.PR, L.M):
        for bad_B, bad_X in ((np.ones(n), X0), (B, np.zeros((2, n - 1))), (np.ones((3, n)), X0)):
            with pytest.raises(ValueError, match=r'shape \(2, %d\)' % n):
                bare.begin_multi(variant, bad_B, bad_X, 5)
    assert 'L.PR' in device.DeviceCSR.begin_multi.__doc__ and 'L.M' in device.DeviceCSR.begin_multi.__doc__
