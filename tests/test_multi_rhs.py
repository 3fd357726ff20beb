"""Two right-hand sides in one Hestenes-Stiefel session (prcg.h: prcg_solve_begin_multi; DeviceCSR.begin_multi;
cg_variants.hs_cg_multi / hs_pcg_multi).

The session runs, per column, exactly the recurrence of hs_cg / hs_pcg, and every inner product is summed in the order
tests/device_order.py: device_sum models.  So the oracle (oracle/ne_oracle.py) run with ``dot=device_dot`` is asked for
EQUAL BITS: vectors, the three inner products of every iteration, both coefficients, the history.  No tolerance anywhere.
The harness shared with the other multi-RHS files: tests/multi_rhs_common.py.

The recorded history is compared with sqrt(device_dot(r_k, r_k)) of the oracle's r_k: the device records the square
root of the r.r it sums (prcg_get_history does the same for single sessions), the oracle's own recorder calls
numpy.linalg.norm, which sums in BLAS order -- another rounding of the same number, so not a bit reference.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import multi_rhs_common as common
from multi_rhs_common import KNOBS, VECS, _raises, amd, operator, same, single_session, two_rhs      # noqa: F401  (amd: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
assert_column_bits = functools.partial(common.assert_column_bits, keys=common.HS_KEYS)


def oracle_column(A, b, x0, iters, jacobi):
    """hs_cg / hs_pcg of the oracle with the device's summation order: the state after `iters` iterations, the scalars
    mu, nu, rr and the coefficients of every iteration, and the history the device records."""
    return common.hs_column(A, b, x0, iters, jacobi, rt_without_jacobi=True)


def device_columns(op, L, B, X0, iters, inv_diag, chunks=(1, 2, 7)):
    """The two-RHS session on `op`: the same quantities per column, read through the per-column getters."""
    def begin():
        op.begin_multi(L.HS, B, X0, iters + 1, inv_diag=inv_diag, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM)
    return common.device_columns(op, L, begin, iters, 2, VECS + (('rt',) if inv_diag is not None else ()), common.served_slots(L, True),
                                 chunks)

# K per operator: 60 where nothing else decides.  s3_small with Jacobi converges until r underflows to exact zeros (the
# ORACLE's nu / mu is 0 / 0 from iteration 49 on): 40 there.  Every case is checked to stay finite in the oracle.
CASES = [(name, jac, 40 if (name, jac) == ('s3_small', True) else 60, False)
         for name in ('s3_small', 's1_small', 'lap3d', 'fem12', 'fem_irregular10', 'bcsstk14', 'bcsstk14_csr')
         for jac in (False, True)] + [('fem12', True, 60, True)]


@pytest.mark.gpu
@pytest.mark.parametrize('name,jacobi,iters,x0_nonzero', CASES)
def test_bits_against_the_device_ordered_oracle(amd, name, jacobi, iters, x0_nonzero):
    """Both columns of a two-RHS session against two oracle runs: x, r, p, s, (rt), mu / nu / rr of every iteration,
    alpha, beta and the history -- equal bits."""
    L, P = amd['L'], amd['problems']
    A, family = operator(name)
    n = A.shape[0]
    B = two_rhs(P, A)
    X0 = np.zeros((2, n))
    if x0_nonzero:
        X0 = np.random.default_rng(11).standard_normal((2, n))
    inv_diag = 1 / A.diagonal() if jacobi else None
    op = amd['device'].DeviceCSR(A, knobs=KNOBS.get(name))
    try:
        got, sched = device_columns(op, L, B, X0, iters, inv_diag)
    finally:
        op.close()
    assert sched['rhs2'] and not sched['small'] and not sched['fused'], sched
    for key, val in family.items():
        assert sched[key] == val, (name, key, sched)
    for j in range(2):
        want = oracle_column(A, B[j], X0[j], iters, jacobi)
        assert np.isfinite(want['scalars']).all() and np.isfinite(want['x']).all(), f'{name}: the oracle run must stay finite'
        assert_column_bits(got[j], want, f'{name} jacobi={jacobi} column {j}')
    print(f'{name} jacobi={jacobi}: n={n}, {iters} iterations, both columns bit-exact; schedule {sched}')


@pytest.mark.gpu
@pytest.mark.parametrize('jacobi', [False, True])
def test_columns_are_independent(amd, jacobi):
    """Swapped right-hand sides give swapped bits, equal ones equal columns, and a column that breaks down at once
    (b = 0, x0 = 0: 0 / 0) leaves the other column's bits alone while its own history holds the NaNs."""
    L, P = amd['L'], amd['problems']
    A, _ = operator('fem12')
    n = A.shape[0]
    B = two_rhs(P, A)
    X0 = np.zeros((2, n))
    inv_diag = 1 / A.diagonal() if jacobi else None
    iters = 25
    op = amd['device'].DeviceCSR(A)
    try:
        ab, _ = device_columns(op, L, B, X0, iters, inv_diag)
        ba, _ = device_columns(op, L, B[::-1], X0, iters, inv_diag)
        aa, _ = device_columns(op, L, np.stack([B[0], B[0]]), X0, iters, inv_diag)
        a0, _ = device_columns(op, L, np.stack([B[0], np.zeros(n)]), X0, iters, inv_diag)
    finally:
        op.close()
    assert_column_bits(ba[1], ab[0], 'swapped: column 1 of (b1, b0) vs column 0 of (b0, b1)')
    assert_column_bits(ba[0], ab[1], 'swapped: column 0 of (b1, b0) vs column 1 of (b0, b1)')
    assert_column_bits(aa[1], aa[0], '(b0, b0): the two columns')
    assert_column_bits(aa[0], ab[0], '(b0, b0) vs (b0, b1): column 0')
    assert_column_bits(a0[0], aa[0], '(b0, 0): column 0 beside a column that broke down')
    assert np.isfinite(a0[0]['hist']).all()
    want = oracle_column(A, np.zeros(n), np.zeros(n), iters, jacobi)
    assert want['hist'][0] == 0.0 and np.isnan(want['hist'][1:]).all()
    assert_column_bits(a0[1], want, '(b0, 0): the column that broke down')


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['HS', 'PIPE_PR'])
@pytest.mark.parametrize('name', ['s3_small', 'fem12'])
def test_single_sessions_did_not_move(amd, variant, name):
    """A single session, a two-RHS session, the same single session again on ONE handle: the two single results are
    bitwise equal, and equal to a fresh handle's -- the new session type leaves nothing behind."""
    L, P = amd['L'], amd['problems']
    A, _ = operator(name)
    n = A.shape[0]
    B = two_rhs(P, A)
    iters = 24
    v = getattr(L, variant)
    op = amd['device'].DeviceCSR(A)
    fresh = amd['device'].DeviceCSR(A)
    try:
        first = single_session(op, L, v, B[0], np.zeros(n), iters)
        device_columns(op, L, B, np.zeros((2, n)), 9, 1 / A.diagonal())
        assert op.schedule()['rhs2']
        again = single_session(op, L, v, B[0], np.zeros(n), iters)
        other = single_session(fresh, L, v, B[0], np.zeros(n), iters)
    finally:
        op.close()
        fresh.close()
    assert not first[0]['rhs2'] and not again[0]['rhs2']
    for run, what in ((again, 'after a two-RHS session'), (other, 'fresh handle')):
        assert run[0] == first[0], (what, run[0], first[0])
        for v_ in VECS:
            assert same(run[1][v_], first[1][v_]), (what, v_)
        assert same(run[2], first[2]) and same(run[3], first[3]) and same(run[4], first[4]), what


@pytest.mark.gpu
def test_refusals(amd):
    """Everything the two-RHS session does not serve is PRCG_EINVAL with a text naming the reason; inside a two-RHS
    session the single-column accessors are refused instead of answering for column 0."""
    L, P, cgv = amd['L'], amd['problems'], amd['cgv']
    A, _ = operator('fem12')
    n = A.shape[0]
    B = two_rhs(P, A)
    X0 = np.zeros((2, n))
    lib = L.lib()
    op = amd['device'].DeviceCSR(A)
    try:
        with _raises(L, 'PRCG_HS'):
            op.begin_multi(L.PIPE_PR, B, X0, 8)
        with _raises(L, 'history bits other than PRCG_HIST_UPDATED_RESIDUAL_2_NORM'):
            op.begin_multi(L.HS, B, X0, 8, hist_mask=L.HIST_RESIDUAL_2_NORM)
        three = (C.c_void_p * 3)(B[0].ctypes.data, B[1].ctypes.data, B[0].ctypes.data)
        rc = lib.prcg_solve_begin_multi(op._h, L.HS, 3, three, three, 8, None, 0)
        assert rc == L.EINVAL and b'nrhs = 3' in lib.prcg_last_error(op._h)
        # a host-callback preconditioner left on the handle
        op.begin(L.HS, B[0], X0[0], 4, preconditioner=lambda v: 0.5 * v[::-1][::-1] + 0.0)
        with _raises(L, 'host-callback preconditioner'):
            op.begin_multi(L.HS, B, X0, 8)
        # block Jacobi left on the handle
        bj = cgv.BlockJacobi(A, 3)
        op.begin(L.HS, B[0], X0[0], 4, block_jacobi=(3, bj.inv_blocks))
        with _raises(L, 'block-Jacobi preconditioner'):
            op.begin_multi(L.HS, B, X0, 8)
        op.clear_preconditioners()
        op.set_replace_hook(lambda k: False)
        with _raises(L, 'replace hook'):
            op.begin_multi(L.HS, B, X0, 8)
        op.set_replace_hook(None)
        # the per-column getters need a two-RHS session
        op.begin(L.HS, B[0], X0[0], 4)
        with _raises(L, 'no open two-RHS session'):
            op.get_vector('x', rhs=0)
        # inside one, the single-column accessors are refused
        op.begin_multi(L.HS, B, X0, 8, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM)
        op.iterate(2)
        for call in (lambda: op.get_vector('x'), lambda: op.set_vector('x', B[0]), lambda: op.get_scalars(1),
                     lambda: op.set_scalars(1, np.zeros(L.NUM_SCALARS)), lambda: op.get_coefficients(1),
                     lambda: op.history(), lambda: op.set_iteration(1)):
            with _raises(L, 'two right-hand sides'):
                call()
        with _raises(L, 'right-hand side 2 out of range'):
            op.get_vector('x', rhs=2)
        with _raises(L, 'not part of the two-RHS session'):
            op.get_vector('rt', rhs=0)           # no Jacobi in this session
        with _raises(L, 'not part of the two-RHS session'):
            op.get_vector('w', rhs=0)
        op.iterate(1)                            # the session is intact after the refusals
        op.sync()
        assert op.k == 3 and np.isfinite(op.get_vector('x', rhs=1)).all()
    finally:
        op.close()
    # ghost columns
    ghost = amd['device'].DeviceCSR(sp.hstack([A, sp.csr_matrix((n, 5))]).tocsr())
    try:
        with _raises(L, 'n_ghost = 5 > 0'):
            ghost.begin_multi(L.HS, B, X0, 8)
    finally:
        ghost.close()


@pytest.mark.gpu
def test_refused_with_a_communicator(amd):
    """A communicator on the handle -- even of one rank -- selects the multi-rank schedules: no two-RHS session."""
    from test_distributed import rccl_ids
    L, P = amd['L'], amd['problems']
    A, _ = operator('fem12')
    n = A.shape[0]
    B, X0 = two_rhs(P, A), np.zeros((2, n))
    uid, path = rccl_ids(1)
    comm = amd['device'].DeviceCSR(A, comm_init=(0, 1, uid, path))
    try:
        with _raises(L, 'communicator'):
            comm.begin_multi(L.HS, B, X0, 8)
    finally:
        comm.close()


@pytest.mark.gpu
def test_hs_cg_multi_returns_two_trials(amd):
    """cg_variants.hs_cg_multi / hs_pcg_multi: two trial dicts shaped like hs_cg's, the histories those of the session;
    Jacobi(A) and a callable that probes as a diagonal are the same session; light host callbacks are called per column."""
    L, P, cgv, cbs = amd['L'], amd['problems'], amd['cgv'], amd['cbs']
    A, _ = operator('fem12')
    n = A.shape[0]
    B = two_rhs(P, A)
    X0 = np.zeros((2, n))
    iters = 30
    seen = []

    def light(**env):
        seen.append((env['output']['rhs'], env['k']))
    light.prcg_host_light = True
    plain = cgv.hs_cg_multi(A, B, X0, iters + 1, callbacks=[cbs.updated_residual_2_norm])
    jac = cgv.hs_pcg_multi(A, B, X0, iters + 1, preconditioner=cgv.Jacobi(A), callbacks=[cbs.updated_residual_2_norm, light])
    d = 1 / A.diagonal()
    probed = cgv.hs_pcg_multi(A, B, X0, iters + 1, preconditioner=lambda v: d * v, callbacks=[cbs.updated_residual_2_norm])
    cgv.clear_operator_cache()
    assert seen == [(j, k) for k in range(iters + 1) for j in range(2)]
    for j in range(2):
        assert plain[j]['name'] == 'hs_cg_multi' and plain[j]['max_iter'] == iters + 1 and jac[j]['name'] == 'hs_pcg_multi'
        for trial, jacobi in ((plain[j], False), (jac[j], True), (probed[j], True)):
            want = oracle_column(A, B[j], X0[j], iters, jacobi)
            assert same(trial['updated_residual_2_norm'], want['hist']), (j, jacobi)


@pytest.mark.gpu
def test_at_size_s4b_80(amd):
    """s4b_80 (n = 1,536,000, 81 nonzeros per row, sliced rows): 5 iterations of a two-RHS session against the oracle,
    bits of x, r and the scalars; the operator's schedule bits are those of a single session."""
    L, P = amd['L'], amd['problems']
    A = P.WORKLOADS['s4b_80']['make']()
    n = A.shape[0]
    B = two_rhs(P, A)
    X0 = np.zeros((2, n))
    iters = 5
    op = amd['device'].DeviceCSR(A)
    try:
        op.begin(L.HS, B[0], X0[0], iters + 1)
        single = op.schedule()
        got, sched = device_columns(op, L, B, X0, iters, None, chunks=(2,))
    finally:
        op.close()
    assert sched['rhs2'] and sched['sliced_rows'] and not sched['small'], sched
    assert sched['stream_stores'] == single['stream_stores'], (sched, single)
    for key in ('sliced_rows', 'nt_loads', 'window_codes', 'sorted_windows', 'col_bytes', 'value_dict'):
        assert sched[key] == single[key], (key, sched, single)
    for j in range(2):
        want = oracle_column(A, B[j], X0[j], iters, False)
        for q in ('x', 'r', 'scalars', 'alpha', 'beta'):
            assert same(got[j][q], want[q]), (j, q)


# ---- no GPU needed ----------------------------------------------------------------------------------------------------
def test_header_binding_and_schedule_bit():
    """The five new entry points are declared, exported and bound (the export test of test_abi_and_planning.py walks
    the header by itself); the schedule bit is the one the header names and collides with no other."""
    from new_cg_variants_amd import _lib as L
    text = open(os.path.join(ROOT, 'include', 'prcg.h')).read()
    lib = L.lib()
    for name in ('prcg_solve_begin_multi', 'prcg_get_vector_rhs', 'prcg_get_scalars_rhs', 'prcg_get_coefficients_rhs',
                 'prcg_get_history_rhs'):
        assert re.search(r'\bint\s+%s\s*\(' % name, text), name
        assert hasattr(lib, name) and name in L._SIGNATURES, name
    bits = {name: int(val) for name, val in re.findall(r'#define\s+(PRCG_SCHED_[A-Z0-9_]+)\s+(\d+)', text)}
    assert bits['PRCG_SCHED_RHS2'] == 16777216
    assert sorted(bits.values()) == sorted(set(bits.values())) and 1048576 not in bits.values()
    assert 'hs_cg.py:9' in text[text.index('TWO right-hand sides'):text.index('prcg_solve_begin_multi(')]


def test_python_argument_checks_come_before_any_device_call(monkeypatch):
    """hs_cg_multi / hs_pcg_multi / begin_multi check shapes and refuse what the session does not serve with
    ValueError -- before an operator is uploaded or a library call is made, and without falling back to two sessions."""
    import new_cg_variants_amd.cg_variants as cgv
    import new_cg_variants_amd.callbacks as cbs
    from new_cg_variants_amd import device, problems as P

    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(cgv, '_operator', no_device)
    monkeypatch.setattr(cgv, 'DeviceCSR', no_device)
    A = P.fem_like_3d(4)
    n = A.shape[0]
    B, X0 = np.ones((2, n)), np.zeros((2, n))
    for bad_B, bad_X in ((np.ones(n), X0), (np.ones((3, n)), np.zeros((3, n))), (np.ones((n, 2)), X0), (B, np.zeros(n)),
                         (np.ones((2, n + 1)), X0)):
        with pytest.raises(ValueError, match=r'shape \(2, %d\)' % n):
            cgv.hs_cg_multi(A, bad_B, bad_X, 5)
    with pytest.raises(ValueError, match='block-Jacobi'):
        cgv.hs_pcg_multi(A, B, X0, 5, preconditioner=cgv.BlockJacobi(A, 3))
    with pytest.raises(ValueError, match='no diagonal scaling'):
        cgv.hs_pcg_multi(A, B, X0, 5, preconditioner=lambda v: np.roll(v, 1))
    with pytest.raises(ValueError, match='hs_pcg_multi'):
        cgv.hs_cg_multi(A, B, X0, 5, preconditioner=cgv.Jacobi(A))
    with pytest.raises(ValueError, match='error_A_norm is not served'):
        cgv.hs_cg_multi(A, B, X0, 5, callbacks=[cbs.error_A_norm])
    with pytest.raises(ValueError, match='needs the state vectors'):
        cgv.hs_cg_multi(A, B, X0, 5, callbacks=[lambda **env: None])
    with pytest.raises(ValueError, match='x_true'):
        cgv.hs_cg_multi(A, B, X0, 5, x_true=np.ones(n))
    # what IS served gets as far as the device
    with pytest.raises(AssertionError, match='the device was reached'):
        cgv.hs_pcg_multi(A, B, X0, 5, preconditioner=cgv.Jacobi(A), callbacks=[cbs.updated_residual_2_norm])
    # DeviceCSR.begin_multi: shapes are checked before the library is called (a bare object has no handle to call with)
    bare = object.__new__(device.DeviceCSR)
    bare.n, bare._lib, bare._h = n, None, None
    for bad_B, bad_X in ((np.ones(n), X0), (B, np.zeros((2, n - 1))), (np.ones((3, n)), X0)):
        with pytest.raises(ValueError, match=r'shape \(2, %d\)' % n):
            bare.begin_multi(0, bad_B, bad_X, 5)
    with pytest.raises(ValueError, match='inv_diag'):
        bare.begin_multi(0, B, X0, 5, inv_diag=np.ones(n + 2))
    assert 'hs_cg_multi' in cgv.__all__ and 'hs_pcg_multi' in cgv.__all__
