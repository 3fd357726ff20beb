"""Two right-hand sides in one PIPELINED predict-and-recompute session (prcg.h: prcg_solve_begin_multi_pipe;
DeviceCSR.begin_multi_pipe; cg_variants.pipe_pr_cg_multi / pipe_pr_pcg_multi / pipe_pr_m_cg_multi / pipe_pr_m_pcg_multi).

The session runs, per column, exactly the recurrence of pipe_pr_cg / pipe_pr_m_cg (pipe_pr_cg.py:9-81; with Jacobi :109-193),
its [w u] = A [r s] of both columns as ONE product of four vectors, and every inner product is summed in the order
tests/device_order.py: device_sum models.  So the oracle (oracle/ne_oracle.py) run with ``dot=device_dot`` and
``square=lambda a: a*a`` (the device multiplies) is asked for EQUAL BITS: vectors, the five inner products of every
iteration, alpha, beta, the predicted nu, the history.  No tolerance anywhere; NaN equals NaN.

The recorded history is compared with sqrt(device_dot(r_k, r_k)) of the oracle's r_k.  The oracle runs are computed once
per (operator, flavour, preconditioner, right-hand side) and shared; nobody writes to them.  The harness shared with the other multi-RHS files:
tests/multi_rhs_common.py.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import multi_rhs_common as common
import oracle.ne_oracle as orc
from device_order import chunking
from multi_rhs_common import KNOBS, _raises, amd, assert_finite, same, single_session      # noqa: F401  (amd: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECS = ('x', 'r', 'p', 's', 'w', 'u')
KEYS = VECS + ('rt', 'st', 'scalars', 'alpha', 'beta', 'nu_pred', 'hist')
NAMES = ('pipe_pr_cg_multi', 'pipe_pr_pcg_multi', 'pipe_pr_m_cg_multi', 'pipe_pr_m_pcg_multi')
assert_column_bits = functools.partial(common.assert_column_bits, keys=KEYS)
single_session = functools.partial(single_session, vecs=VECS)


def oracle_column(A, b, x0, iters, jacobi, flavour='pr'):
    """pipe_pr_cg / pipe_pr_pcg / pipe_pr_m_cg / pipe_pr_m_pcg of the oracle with the device's summation order and its a * a:
    the state after `iters` iterations, mu, delta, gamma, nu, rr of every iteration, the coefficients used BY every
    iteration >= 1, the recorded history."""
    method = {('pr', False): orc.pipe_pr_cg, ('pr', True): orc.pipe_pr_pcg,
              ('pr_m', False): orc.pipe_pr_m_cg, ('pr_m', True): orc.pipe_pr_m_pcg}[(flavour, jacobi)]
    return common.oracle_column(method, A, b, x0, iters, vecs=VECS, tilde=('rt', 'st') if jacobi else (),
                                preconditioner=orc.jacobi(A) if jacobi else None, dot=common.dot, square=lambda a: a * a)


def device_columns(op, L, variant, B, X0, iters, inv_diag, chunks=(1, 2, 7)):
    """A pipelined two-RHS session of `variant` on `op`, read through the per-column getters: per column the vectors, ALL
    scalar slots of every iteration, the three coefficients of every iteration >= 1 and the history; and the schedule."""
    def begin():
        op.begin_multi_pipe(variant, B, X0, iters + 1, inv_diag=inv_diag, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM)
    return common.device_columns(op, L, begin, iters, 2, VECS + (('rt', 'st') if inv_diag is not None else ()),
                                 common.served_slots(L, False), chunks)


# The pipelined session's product is the four-vector one: ONE launch on sliced rows, which its schedule() reports beside the shared
# `family` keys (a two-RHS Hestenes-Stiefel session on the same operator reports spmm4 false)
SPMM4 = {'s3_small': False, 'lap3d': False, 'fem12': True, 'fem_irregular10': True, 'bcsstk14': True, 'bcsstk14_csr': False}


# ... and the sizes at which the update kernel can go wrong: this file's own operators, tridiag<n>
SIZES = [63, 64, 255, 257, 511, 513, 1025, 2049]
common.OPERATORS.update({f'tridiag{n}': (functools.partial(sp.diags, [-1.0, 2.5, -1.0], [-1, 0, 1], shape=(n, n), format='csr'), {})
                         for n in SIZES})


def operator(name):
    """One operator per product family of the multi-vector products; `family` is asserted through schedule()."""
    A, family = common.operator(name)
    return A, dict(family, **({'spmm4': SPMM4[name]} if name in SPMM4 else {}))


def problem(name, x0_nonzero=False):
    """(A, B, X0) of an operator"""
    return common.problem(name, 2, x0_nonzero)


# reference(name, flavour, jacobi, iters, x0_nonzero, column): the oracle run of one column, computed once and shared (read-only).
# column: 0, 1, or 'zero' (b = 0, x0 = 0)
reference = functools.partial(common.reference, oracle_column, 2)

def variant_of(L, flavour):
    return {'pr': L.PIPE_PR, 'pr_m': L.PIPE_PR_M}[flavour]


# K per case: 60 where nothing else decides.  s3_small with Jacobi: pipe_pr_m_pcg of the oracle breaks down at iteration 6 on
# that diagonally dominant band, so 5 there for both flavours.  Every case asserts its oracle run finite, mu, nu > 0.
def _iters(name, jacobi):
    return 5 if (name, jacobi) == ('s3_small', True) else 60


CASES = ([('pr', name, jac, _iters(name, jac), False)
          for name in ('s3_small', 'lap3d', 'fem12', 'fem_irregular10', 'bcsstk14', 'bcsstk14_csr')
          for jac in (False, True)]
         + [('pr_m', name, jac, _iters(name, jac), False) for name in ('s3_small', 'fem12', 'bcsstk14') for jac in (False, True)]
         + [('pr', 'fem12', True, 60, True)])


# ---- 1. bits against the device-ordered oracle ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('flavour,name,jacobi,iters,x0_nonzero', CASES)
def test_bits_against_the_device_ordered_oracle(amd, flavour, name, jacobi, iters, x0_nonzero):
    """Both columns of a pipelined two-RHS session against two oracle runs: x, r, p, s, w, u, (rt, st), mu / delta / gamma /
    nu / rr of every iteration, alpha, beta, the predicted nu and the history -- equal bits."""
    L = amd['L']
    matrix = 'bcsstk14' if name == 'bcsstk14_csr' else name          # the same matrix, another product family: one oracle run
    A, B, X0 = problem(matrix, x0_nonzero)
    _, family = operator(name)
    n = A.shape[0]
    want = [reference(matrix, flavour, jacobi, iters, x0_nonzero, j) for j in range(2)]
    for j in range(2):
        assert_finite(want[j], f'{flavour} {name} jacobi={jacobi} column {j}')
    inv_diag = 1 / A.diagonal() if jacobi else None
    op = amd['device'].DeviceCSR(A, knobs=KNOBS.get(name))
    try:
        got, sched = device_columns(op, L, variant_of(L, flavour), B, X0, iters, inv_diag)
    finally:
        op.close()
    assert sched['rhs2'] and sched['rhs2_pipe'] and not sched['rhs4'] and not sched['small'] and not sched['fused'], sched
    for key, val in family.items():
        assert sched[key] == val, (name, key, sched)
    for j in range(2):
        assert_column_bits(got[j], want[j], f'{flavour} {name} jacobi={jacobi} column {j}')
    print(f'{flavour} {name} jacobi={jacobi}: n={n}, {iters} iterations, both columns bit-exact; schedule {sched}')


# ---- 2. sizes at which the update kernel can go wrong ---------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('jacobi', [False, True])
@pytest.mark.parametrize('n', SIZES)
def test_update_kernel_sizes(amd, n, jacobi):
    """A lane with only its first element (n <= 256), a ragged second half, one block and several: both flavours, 5 iterations."""
    L = amd['L']
    name = f'tridiag{n}'
    A, B, X0 = problem(name)
    assert A.shape == (n, n)
    iters = 5
    inv_diag = 1 / A.diagonal() if jacobi else None
    op = amd['device'].DeviceCSR(A)
    try:
        for flavour in ('pr', 'pr_m'):
            want = [reference(name, flavour, jacobi, iters, False, j) for j in range(2)]
            for j in range(2):
                assert_finite(want[j], f'{flavour} n={n} jacobi={jacobi} column {j}')
            got, sched = device_columns(op, L, variant_of(L, flavour), B, X0, iters, inv_diag, chunks=(2,))
            assert sched['rhs2_pipe'] and not sched['small'], sched
            for j in range(2):
                assert_column_bits(got[j], want[j], f'{flavour} n={n} jacobi={jacobi} column {j}')
    finally:
        op.close()


@pytest.mark.gpu
def test_two_trips_per_block(amd):
    """laplace_3d(102, 102, 101): n = 1,050,804 > 2048 * 512, chunking(n) = (1027, 2) -- the smallest shape at which the update
    kernel's trip loop, its `base >= n` exit and its ragged last block run.  pr, without and with Jacobi, 3 iterations."""
    L = amd['L']
    A, B, X0 = problem('lap3d_two_trips')
    n = A.shape[0]
    assert n == 1050804 and chunking(n) == (1027, 2)
    iters = 3
    op = amd['device'].DeviceCSR(A)
    try:
        for jacobi in (False, True):
            want = [reference('lap3d_two_trips', 'pr', jacobi, iters, False, j) for j in range(2)]
            for j in range(2):
                assert_finite(want[j], f'two trips, jacobi={jacobi}, column {j}')
            got, sched = device_columns(op, L, L.PIPE_PR, B, X0, iters, 1 / A.diagonal() if jacobi else None, chunks=(2, 1))
            assert sched['rhs2_pipe'] and not sched['small'] and not sched['fused'], sched
            for j in range(2):
                assert_column_bits(got[j], want[j], f'two trips, jacobi={jacobi}, column {j}')
    finally:
        op.close()


# ---- 3. device against device -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('jacobi', [False, True])
@pytest.mark.parametrize('name', ['s3_small', 'fem12'])
def test_columns_equal_single_two_kernel_sessions(amd, name, jacobi):
    """Column j of the session equals a single session of the same variant opened with PRCG_FUSED=0 -- the two-kernel schedule:
    the same expressions, the same tree.  After 20 iterations: x, r, p, s, w, u, the five scalars of every iteration, a, b and
    the predicted nu."""
    L = amd['L']
    A, B, X0 = problem(name)
    iters = 20
    inv_diag = 1 / A.diagonal() if jacobi else None
    op = amd['device'].DeviceCSR(A)
    single = amd['device'].DeviceCSR(A, knobs={'PRCG_FUSED': '0'})
    try:
        for flavour in ('pr', 'pr_m'):
            variant = variant_of(L, flavour)
            got, _ = device_columns(op, L, variant, B, X0, iters, inv_diag)
            for j in range(2):
                sched, vec, sc, cf, hist = single_session(single, L, variant, B[j], X0[j], iters, inv_diag)
                assert not sched['fused'] and not sched['small'] and not sched['rhs2'], sched
                what = f'{name} {flavour} jacobi={jacobi} column {j}'
                for v in VECS:
                    assert same(got[j][v], vec[v]), (what, v)
                assert same(got[j]['scalars'], sc[:, :5]), what
                assert same(np.stack([got[j]['alpha'], got[j]['beta'], got[j]['nu_pred']], axis=1), cf), what
                assert same(got[j]['hist'], hist), what
    finally:
        op.close()
        single.close()


# ---- 4. columns are independent -------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('jacobi', [False, True])
def test_columns_are_independent(amd, jacobi):
    """Swapped right-hand sides give swapped bits, and a column that breaks down at once (b = 0, x0 = 0: 0 / 0) leaves the other
    column's bits alone while its own history holds the NaNs."""
    L = amd['L']
    A, B, X0 = problem('fem12')
    n = A.shape[0]
    inv_diag = 1 / A.diagonal() if jacobi else None
    iters = 25
    op = amd['device'].DeviceCSR(A)
    try:
        ab, sched = device_columns(op, L, L.PIPE_PR, B, X0, iters, inv_diag)
        ba, _ = device_columns(op, L, L.PIPE_PR, B[::-1], X0, iters, inv_diag)
        a0, _ = device_columns(op, L, L.PIPE_PR, np.stack([B[0], np.zeros(n)]), X0, iters, inv_diag)
    finally:
        op.close()
    assert sched['spmm4'], sched
    assert_column_bits(ba[1], ab[0], 'swapped: column 1 of (b1, b0) vs column 0 of (b0, b1)')
    assert_column_bits(ba[0], ab[1], 'swapped: column 0 of (b1, b0) vs column 1 of (b0, b1)')
    assert_column_bits(a0[0], ab[0], '(b0, 0): column 0 beside a column that broke down')
    assert np.isfinite(a0[0]['hist']).all()
    assert_column_bits(ab[0], reference('fem12', 'pr', jacobi, iters, False, 0), 'column 0 vs the oracle')
    want = reference('fem12', 'pr', jacobi, iters, False, 'zero')
    assert want['hist'][0] == 0.0 and np.isnan(want['hist'][1:]).all()
    assert_column_bits(a0[1], want, '(b0, 0): the column that broke down')


# ---- 5. one product, same bits --------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('jacobi', [False, True])
def test_one_launch_and_two_launch_products_give_the_same_bits(amd, jacobi):
    """fem12: the session whose product is ONE four-vector launch and the one with PRCG_SPMM4=0 (two two-vector launches)."""
    L = amd['L']
    A, B, X0 = problem('fem12')
    inv_diag = 1 / A.diagonal() if jacobi else None
    iters = 30
    one = amd['device'].DeviceCSR(A)
    two = amd['device'].DeviceCSR(A, knobs={'PRCG_SPMM4': '0'})
    try:
        got1, sched1 = device_columns(one, L, L.PIPE_PR, B, X0, iters, inv_diag)
        got2, sched2 = device_columns(two, L, L.PIPE_PR, B, X0, iters, inv_diag)
    finally:
        one.close()
        two.close()
    assert sched1['spmm4'] and not sched2['spmm4'] and sched1['rhs2_pipe'] and sched2['rhs2_pipe'], (sched1, sched2)
    for j in range(2):
        for q in KEYS + ('all_scalars',):
            if got1[j][q] is None:
                assert got2[j][q] is None
            else:
                assert same(got1[j][q], got2[j][q]), (j, q)


# ---- 6. nothing left behind -----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('single', ['PIPE_PR', 'HS'])
@pytest.mark.parametrize('name', ['s3_small', 'fem12'])
def test_nothing_left_behind(amd, name, single):
    """On ONE handle: a single session, the pipelined two-RHS session (with Jacobi), the same single session again.  The single
    runs are bitwise equal, report the same schedule, and equal a fresh handle's."""
    L = amd['L']
    A, B, X0 = problem(name)
    n = A.shape[0]
    variant = getattr(L, single)
    vecs = ('x', 'r', 'p', 's')
    iters, multi_iters = 24, 5
    d = 1 / A.diagonal()
    op = amd['device'].DeviceCSR(A)
    fresh = amd['device'].DeviceCSR(A)
    try:
        first = single_session(op, L, variant, B[0], np.zeros(n), iters, vecs=vecs)
        between, sched = device_columns(op, L, L.PIPE_PR, B, X0, multi_iters, d)
        again = single_session(op, L, variant, B[0], np.zeros(n), iters, vecs=vecs)
        other = single_session(fresh, L, variant, B[0], np.zeros(n), iters, vecs=vecs)
    finally:
        op.close()
        fresh.close()
    assert sched['rhs2'] and sched['rhs2_pipe']
    assert not first[0]['rhs2'] and not first[0]['rhs2_pipe'] and not first[0]['spmm4']
    for run, what in ((again, 'after the pipelined two-RHS session'), (other, 'fresh handle')):
        assert run[0] == first[0], (what, run[0], first[0])
        for v_ in vecs:
            assert same(run[1][v_], first[1][v_]), (what, v_)
        assert same(run[2], first[2]) and same(run[3], first[3]) and same(run[4], first[4]), what
    for j in range(2):
        assert_column_bits(between[j], reference(name, 'pr', True, multi_iters, False, j), f'{name}: the session in between, column {j}')


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(amd):
    """What the pipelined two-RHS session does not serve is PRCG_EINVAL with a text naming the reason; a refused begin leaves an
    open session iterating; the getters refuse wt / ut and j = 2; the single-column accessors are refused while it is open."""
    L, cgv = amd['L'], amd['cgv']
    A, B, X0 = problem('fem12')
    n = A.shape[0]
    d = 1 / A.diagonal()
    lib = L.lib()
    op = amd['device'].DeviceCSR(A)

    def begin(variant, nrhs=2, b=None, x0=None, hist_mask=0):
        bp = b if b is not None else (C.c_void_p * 4)(*[B[j % 2].ctypes.data for j in range(4)])
        xp = x0 if x0 is not None else (C.c_void_p * 4)(*[X0[j % 2].ctypes.data for j in range(4)])
        rc = lib.prcg_solve_begin_multi_pipe(op._h, variant, nrhs, bp, xp, 8, None, hist_mask)
        return rc, lib.prcg_last_error(op._h).decode()

    try:
        # an open session that every refusal below must leave as it is
        op.begin_multi_pipe(L.PIPE_PR, B, X0, 12, inv_diag=d, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM)
        op.iterate(2)
        for v in (L.PIPE_P, L.PIPE_P_M):
            rc, text = begin(v)
            assert rc == L.EINVAL and 'stored-w flavours' in text and 'not served' in text, text
        for v in (L.HS, L.PR, L.M, L.CG_CG, L.GV, 99, -1):
            rc, text = begin(v)
            assert rc == L.EINVAL and 'serves PRCG_PIPE_PR' in text and 'PRCG_PIPE_PR_M' in text and 'only' in text, text
        for nrhs in (1, 3, 4):
            rc, text = begin(L.PIPE_PR, nrhs=nrhs)
            assert rc == L.EINVAL and f'nrhs = {nrhs}' in text and 'eight-vector product does not exist' in text, text
        rc, text = begin(L.PIPE_PR, hist_mask=L.HIST_RESIDUAL_2_NORM)
        assert rc == L.EINVAL and 'history bits other than PRCG_HIST_UPDATED_RESIDUAL_2_NORM' in text, text
        rc, text = begin(L.PIPE_PR, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM | L.HIST_ERROR_A_NORM)
        assert rc == L.EINVAL and 'history bits other than PRCG_HIST_UPDATED_RESIDUAL_2_NORM' in text, text
        for b_, x_ in ((None, (C.c_void_p * 2)(X0[0].ctypes.data, None)), ((C.c_void_p * 2)(None, B[1].ctypes.data), None)):
            rc, text = begin(L.PIPE_PR_M, b=b_, x0=x_)
            assert rc == L.EINVAL and 'null b or x0' in text, text
        rc = lib.prcg_solve_begin_multi_pipe(op._h, L.PIPE_PR, 2, None, None, 8, None, 0)
        assert rc == L.EINVAL and b'null b or x0' in lib.prcg_last_error(op._h)
        # ... the session is still open, is still the pipelined one and goes on
        sched = op.schedule()
        assert sched['rhs2'] and sched['rhs2_pipe']
        op.iterate(3)
        op.sync()
        want = reference('fem12', 'pr', True, 5, False, 1)
        assert op.k == 5 and same(op.get_vector('x', rhs=1), want['x']) and same(op.get_vector('u', rhs=1), want['u'])
        # the getters
        for name in ('wt', 'ut'):
            with _raises(L, 'not part of the pipelined two-RHS session'):
                op.get_vector(name, rhs=0)
        with _raises(L, 'right-hand side 2 out of range'):
            op.get_vector('x', rhs=2)
        with _raises(L, 'right-hand side 2 out of range'):
            op.get_scalars(1, rhs=2)
        with _raises(L, 'right-hand side 2 out of range'):
            op.get_coefficients(1, rhs=2)
        with _raises(L, 'right-hand side 2 out of range'):
            op.history(rhs=2)
        for call in (lambda: op.get_vector('x'), lambda: op.set_vector('x', B[0]), lambda: op.get_scalars(1),
                     lambda: op.set_scalars(1, np.zeros(L.NUM_SCALARS)), lambda: op.get_coefficients(1),
                     lambda: op.history(), lambda: op.set_iteration(1)):
            with _raises(L, 'two right-hand sides'):
                call()
        op.iterate(1)
        op.sync()
        assert op.k == 6 and np.isfinite(op.get_vector('x', rhs=0)).all()
        # without Jacobi rt and st are no part of the session
        op.begin_multi_pipe(L.PIPE_PR_M, B, X0, 8)
        for name in ('rt', 'st', 'wt', 'ut'):
            with _raises(L, 'not part of the pipelined two-RHS session'):
                op.get_vector(name, rhs=1)
        # begin_multi keeps refusing the pipelined variants, in its own words
        with _raises(L, r'PRCG_HS \(hs_cg / hs_pcg\), PRCG_PR \(pr_cg / pr_pcg\) and PRCG_M \(m_cg / m_pcg\) only'):
            op.begin_multi(L.PIPE_PR, B, X0, 8)
        # a host-callback preconditioner left on the handle
        op.begin(L.PIPE_PR, B[0], X0[0], 4, preconditioner=lambda v: 0.5 * v[::-1][::-1] + 0.0)
        with _raises(L, 'host-callback preconditioner'):
            op.begin_multi_pipe(L.PIPE_PR, B, X0, 8)
        op.iterate(1)                            # the single session the refusal left open
        op.sync()
        assert op.k == 1 and not op.schedule()['rhs2']
        # block Jacobi left on the handle
        bj = cgv.BlockJacobi(A, 3)
        op.begin(L.PIPE_PR, B[0], X0[0], 4, block_jacobi=(3, bj.inv_blocks))
        with _raises(L, 'block-Jacobi preconditioner'):
            op.begin_multi_pipe(L.PIPE_PR_M, B, X0, 8)
        op.clear_preconditioners()
        op.set_replace_hook(lambda k: False)
        with _raises(L, 'replace hook'):
            op.begin_multi_pipe(L.PIPE_PR, B, X0, 8)
        op.set_replace_hook(None)
        # ... and afterwards the handle opens the session again, and an ordinary two-RHS session after it
        op.begin_multi_pipe(L.PIPE_PR, B, X0, 8)
        op.iterate(2)
        op.begin_multi(L.PR, B, X0, 8)
        sched = op.schedule()
        assert sched['rhs2'] and not sched['rhs2_pipe'] and not sched['spmm4'], sched
        op.iterate(2)
        op.sync()
        assert same(op.get_vector('x', rhs=0), _pr_reference_x(A, B[0], X0[0]))
    finally:
        op.close()
    # ghost columns
    ghost = amd['device'].DeviceCSR(sp.hstack([A, sp.csr_matrix((n, 5))]).tocsr())
    try:
        with _raises(L, 'n_ghost = 5 > 0'):
            ghost.begin_multi_pipe(L.PIPE_PR, B, X0, 8)
    finally:
        ghost.close()


def _pr_reference_x(A, b, x0):
    """x after two iterations of the oracle's identity-preconditioned pr_pcg with the device's sums"""
    with np.errstate(all='ignore'):
        out = orc.pr_pcg(A, b, x0, 3, preconditioner=lambda v: v, dot=common.dot, square=lambda a: a * a)
    return out['_final_state'].x


@pytest.mark.gpu
def test_refused_with_a_communicator(amd):
    """A communicator on the handle -- even of one rank -- selects the multi-rank schedules: no pipelined two-RHS session."""
    from test_distributed import rccl_ids
    L = amd['L']
    A, B, X0 = problem('fem12')
    uid, path = rccl_ids(1)
    comm = amd['device'].DeviceCSR(A, comm_init=(0, 1, uid, path))
    try:
        with _raises(L, 'communicator is set on the handle'):
            comm.begin_multi_pipe(L.PIPE_PR, B, X0, 8)
    finally:
        comm.close()


# ---- 8. public functions --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_public_function_returns_two_trials(amd):
    """pipe_pr_pcg_multi on fem12: two trial dicts named after the function, the histories those of the oracle's columns."""
    cgv, cbs = amd['cgv'], amd['cbs']
    A, B, X0 = problem('fem12')
    iters = 39
    try:
        trials = cgv.pipe_pr_pcg_multi(A, B, X0, iters + 1, preconditioner=cgv.Jacobi(A), callbacks=[cbs.updated_residual_2_norm])
    finally:
        cgv.clear_operator_cache()
    assert len(trials) == 2
    for j in range(2):
        assert trials[j]['name'] == 'pipe_pr_pcg_multi' and trials[j]['max_iter'] == iters + 1 and trials[j]['rhs'] == j
        want = reference('fem12', 'pr', True, iters, False, j)
        assert np.isfinite(want['hist']).all()
        assert same(trials[j]['updated_residual_2_norm'], want['hist']), j
    # the histories carry the bits of case 1 (60 iterations of the same recurrence): its first 40 entries
    for j in range(2):
        assert same(trials[j]['updated_residual_2_norm'], reference('fem12', 'pr', True, 60, False, j)['hist'][:iters + 1]), j


# ---- no GPU needed --------------------------------------------------------------------------------------------------------
def test_names_header_and_binding():
    """The four functions are public; the entry point is declared with the reference lines it replaces and bound; the schedule
    bit is the one the header names and collides with no other."""
    import new_cg_variants_amd.cg_variants as cgv
    from new_cg_variants_amd import _lib as L, device
    for name in NAMES:
        assert name in cgv.__all__ and callable(getattr(cgv, name)) and getattr(cgv, name).__name__ == name
    text = open(os.path.join(ROOT, 'include', 'prcg.h')).read()
    assert re.search(r'\bint\s+prcg_solve_begin_multi_pipe\s*\(\s*prcg_t\s*\*\s*h\s*,\s*int\s+variant\s*,\s*int\s+nrhs\s*,\s*const\s+double\s*\*\s*'
                     r'const\s*\*\s*b\s*,\s*const\s+double\s*\*\s*const\s*\*\s*x0\s*,\s*int\s+max_iter\s*,\s*const\s+double\s*\*\s*inv_diag\s*,'
                     r'\s*uint32_t\s+hist_mask\s*\)', text)
    section = text[text.index('pipelined predict-and-recompute with TWO right-hand sides'):text.index('prcg_solve_begin_multi_pipe(')]
    for word in ('PRCG_PIPE_PR', 'PRCG_PIPE_PR_M', 'pipe_pr_cg.py:89', ':201', ':101', ':213', 'PRCG_SCHED_RHS2_PIPE'):
        assert word in section, word
    assert 'prcg_solve_begin_multi_pipe' in L._SIGNATURES and hasattr(L.lib(), 'prcg_solve_begin_multi_pipe')
    bits = {name: int(val) for name, val in re.findall(r'#define\s+(PRCG_SCHED_[A-Z0-9_]+)\s+(\d+)', text)}
    assert bits['PRCG_SCHED_RHS2_PIPE'] == 134217728
    assert sorted(bits.values()) == sorted(set(bits.values())) and 1048576 not in bits.values()
    assert 'L.PIPE_PR' in device.DeviceCSR.begin_multi_pipe.__doc__ and 'L.PIPE_PR_M' in device.DeviceCSR.begin_multi_pipe.__doc__


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
        with pytest.raises(ValueError, match=r'%s: .*exactly two right-hand sides, shape \(2, %d\)' % (name, n)):
            f(A, np.ones((4, n)), np.zeros((4, n)), 5)
        for bad_B, bad_X in ((np.ones(n), X0), (np.ones((3, n)), np.zeros((3, n))), (np.ones((n, 2)), X0), (B, np.zeros(n)),
                             (np.ones((2, n + 1)), X0), (B, np.zeros((4, n)))):
            with pytest.raises(ValueError, match=r'%s: .* shape \(2, %d\)' % (name, n)):
                f(A, bad_B, bad_X, 5)
        with pytest.raises(ValueError, match='x_true'):
            f(A, B, X0, 5, x_true=np.ones(n))
        for rec in (cbs.error_A_norm, cbs.error_2_norm, cbs.residual_2_norm):
            with pytest.raises(ValueError, match='is not served by the two-RHS session'):
                f(A, B, X0, 5, callbacks=[rec])
        with pytest.raises(ValueError, match='needs the state vectors'):
            f(A, B, X0, 5, callbacks=[lambda **env: None])
        # what IS served gets as far as the device
        with pytest.raises(AssertionError, match='the device was reached'):
            f(A, B, X0, 5, callbacks=[cbs.updated_residual_2_norm])
    for name in ('pipe_pr_pcg_multi', 'pipe_pr_m_pcg_multi'):
        f = getattr(cgv, name)
        with pytest.raises(ValueError, match='block-Jacobi'):
            f(A, B, X0, 5, preconditioner=cgv.BlockJacobi(A, 3))
        with pytest.raises(ValueError, match='no diagonal scaling'):
            f(A, B, X0, 5, preconditioner=lambda v: np.roll(v, 1))
        with pytest.raises(AssertionError, match='the device was reached'):
            f(A, B, X0, 5, preconditioner=cgv.Jacobi(A), callbacks=[cbs.updated_residual_2_norm])
    with pytest.raises(ValueError, match='pipe_pr_pcg_multi'):
        cgv.pipe_pr_cg_multi(A, B, X0, 5, preconditioner=cgv.Jacobi(A))
    with pytest.raises(ValueError, match='pipe_pr_m_pcg_multi'):
        cgv.pipe_pr_m_cg_multi(A, B, X0, 5, preconditioner=cgv.Jacobi(A))
    # DeviceCSR: shapes are checked before the library is called; begin_multi_pipe takes exactly two systems
    bare = object.__new__(device.DeviceCSR)
    bare.n, bare._lib, bare._h = n, None, None
    for variant in (L.PIPE_PR, L.PIPE_PR_M):
        for bad_B, bad_X in ((np.ones(n), X0), (B, np.zeros((2, n - 1))), (np.ones((3, n)), X0), (np.ones((4, n)), np.zeros((4, n)))):
            with pytest.raises(ValueError, match=r'shape \(2, %d\)' % n):
                bare.begin_multi_pipe(variant, bad_B, bad_X, 5)
