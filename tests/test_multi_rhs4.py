"""Four right-hand sides in one session over a four-vector product (prcg.h: prcg_solve_begin_multi with nrhs = 4,
prcg_spmm4; DeviceCSR.begin_multi / matmat4; cg_variants.*_multi with (4, n) arrays).

A four-RHS session is two PAIR GROUPS -- columns (0, 1) and (2, 3), each a complete two-RHS state iterated by the two-RHS
vector kernels -- around ONE product [S0 S1 | S2 S3] = A [P0 P1 | P2 P3]: a single launch that reads the operator once on
sliced-row operators (schedule()['spmm4']), two two-vector launches on every other operator or with PRCG_SPMM4=0.

Everything is asked for EQUAL BITS, as in tests/test_multi_rhs.py and tests/test_multi_rhs_pr.py, with the helpers and
operators all of them share (tests/multi_rhs_common.py): the product per column against scipy's csr_matvec and against matmat2 of its pair, the sessions
against the device-ordered oracle and against two two-RHS sessions.  No tolerance anywhere.

Right-hand sides: reference_rhs(A, n)[0] and default_rng(s).standard_normal(n) for s = 7, 8, 9 (columns 0 and 1 are those of
the two-RHS tests).  The oracle runs are computed once per (operator, variant, preconditioner, column) and shared.
"""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import multi_rhs_common as common
from multi_rhs_common import KNOBS, VECS, _raises, amd, assert_finite, four_rhs, operator, same, single_session      # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERM = (2, 0, 3, 1)


def problem(name, x0_nonzero=False):
    return common.problem(name, 4, x0_nonzero)


def oracle_column(A, b, x0, iters, jacobi, variant):
    """One column of the oracle with the device's summation order, in the keys of a predict-and-recompute column; a
    Hestenes-Stiefel column has no delta, gamma, predicted nu or st (and, here, no rt without Jacobi)."""
    if variant != 'hs':
        return common.pr_column(A, b, x0, iters, jacobi, variant)
    return common.hs_column(A, b, x0, iters, jacobi, rt_without_jacobi=False)


# reference(name, variant, jacobi, iters, x0_nonzero, column): the oracle run of one column, computed once and shared (read-only).
# column: 0 .. 3, or 'zero' (b = 0, x0 = 0)
reference = functools.partial(common.reference, oracle_column, 4)


def check_finite(want, variant, what):
    """a case whose oracle run breaks down is a wrong case: it fails, it is not skipped"""
    if variant == 'hs':
        assert np.isfinite(want['scalars']).all() and np.isfinite(want['x']).all(), f'{what}: the oracle run must stay finite'
    else:
        assert_finite(want, what)


def assert_column_bits(got, want, variant, what):
    common.assert_column_bits(got, want, what, common.HS_KEYS if variant == 'hs' else common.KEYS)


def device_columns(op, L, variant, B, X0, iters, inv_diag, chunks=(1, 2, 7)):
    """A multi-RHS session of `variant` ('hs', 'pr', 'm') on `op` with as many columns as B has rows, read through the
    per-column getters: per column the vectors, the served scalars of every iteration, the coefficients, the history."""
    def begin():
        op.begin_multi({'hs': L.HS, 'pr': L.PR, 'm': L.M}[variant], B, X0, iters + 1, inv_diag=inv_diag,
                       hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM)
    tilde = () if inv_diag is None else ('rt',) if variant == 'hs' else ('rt', 'st')
    cols, sched = common.device_columns(op, L, begin, iters, len(B), VECS + tilde, common.served_slots(L, variant == 'hs'), chunks)
    if variant == 'hs':
        assert not any(col['nu_pred'].any() for col in cols), 'Hestenes-Stiefel predicts no nu'
    return cols, sched


def assert_columns_equal(got, want, what):
    """two device columns, every output: vectors, scalars, coefficients, history"""
    assert got.keys() == want.keys(), what
    for q in got:
        if want[q] is None:
            assert got[q] is None, (what, q)
        else:
            assert same(got[q], want[q]), (what, q)


# ---- no GPU needed ----------------------------------------------------------------------------------------------------
def test_arguments_without_device(monkeypatch):
    """(4, n) right-hand sides get as far as the device; every other shape is a ValueError with the shape text before it; the
    new entry point and the two schedule bits are declared."""
    import new_cg_variants_amd.cg_variants as cgv
    from new_cg_variants_amd import _lib as L, problems as P

    def reached(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(cgv, '_operator', reached)
    monkeypatch.setattr(cgv, 'DeviceCSR', reached)
    A = P.fem_like_3d(12)
    n = A.shape[0]
    with pytest.raises(AssertionError, match='the device was reached'):
        cgv.hs_cg_multi(A, np.ones((4, n)), np.zeros((4, n)), 5)
    with pytest.raises(AssertionError, match='the device was reached'):
        cgv.hs_cg_multi(A, np.ones((2, n)), np.zeros((2, n)), 5)
    for bad_B, bad_X in ((np.ones((3, n)), np.zeros((3, n))), (np.ones((5, n)), np.zeros((5, n))), (np.ones((4, n)), np.zeros((2, n))),
                         (np.ones((2, n)), np.zeros((4, n))), (np.ones((4, n + 1)), np.zeros((4, n + 1)))):
        for f in (cgv.hs_cg_multi, cgv.pr_pcg_multi, cgv.m_cg_multi):
            with pytest.raises(ValueError, match=r'shape \(2, %d\) or \(4, %d\)' % (n, n)):
                f(A, bad_B, bad_X, 5)
    text = open(os.path.join(ROOT, 'include', 'prcg.h')).read()
    assert re.search(r'\bint\s+prcg_spmm4\s*\(\s*prcg_t\s*\*\s*h\s*,\s*const\s+double\s*\*\s*x4\s*,\s*double\s*\*\s*y4\s*,\s*int\s+reps\s*,'
                     r'\s*double\s*\*\s*ms_avg\s*\)', text)
    assert 'prcg_spmm4' in L._SIGNATURES
    bits = {name: int(val) for name, val in re.findall(r'#define\s+(PRCG_SCHED_[A-Z0-9_]+)\s+(\d+)', text)}
    assert bits['PRCG_SCHED_RHS4'] == 33554432 and bits['PRCG_SCHED_SPMM4'] == 67108864 and bits['PRCG_SCHED_RHS2'] == 16777216
    assert sorted(bits.values()) == sorted(set(bits.values()))
    assert re.search(r'\bint\s+prcg_version\b', text)


# ---- 1. the product, bit for bit ----------------------------------------------------------------------------------------
def four_columns(rng, n):
    x = rng.standard_normal(n)
    return np.stack([x, 3.0 * x[::-1], rng.standard_normal(n), -0.5 * x], axis=1)


def product_bits(amd, A, X, knobs, family, what, equal_nan=False):
    """matmat4 per column against scipy and against matmat2 of the column's pair; again with PRCG_SPMM4=0: equal bits, and the
    schedule's family is the one the case is meant for.  Returns the product."""
    with np.errstate(all='ignore'):
        ref = np.stack([A @ X[:, c] for c in range(4)], axis=1)
    out = []
    for spmm4 in ('1', '0'):
        op = amd['device'].DeviceCSR(A, knobs=dict(knobs, PRCG_SPMM4=spmm4))
        try:
            s = op.schedule()
            for key, val in family.items():
                assert s[key] == val, (what, key, s)
            Y, _ = op.matmat4(X)
            pairs = np.concatenate([op.matmat2(np.ascontiguousarray(X[:, 2 * g:2 * g + 2]))[0] for g in range(2)], axis=1)
        finally:
            op.close()
        for c in range(4):
            assert np.array_equal(Y[:, c], ref[:, c], equal_nan=equal_nan), (what, spmm4, 'scipy', c)
            assert np.array_equal(Y[:, c], pairs[:, c], equal_nan=equal_nan), (what, spmm4, 'matmat2', c)
        out.append(Y)
    assert np.array_equal(out[0], out[1], equal_nan=equal_nan), what
    return out[0]


def damaged_fem():
    """fem_like_3d(14, 3) of test_sliced_rows_with_window_codes: empty rows, a whole empty slice, runs in descending order"""
    from new_cg_variants_amd import problems as P
    rng = np.random.default_rng(5)
    A = P.fem_like_3d(14, 3).tolil()
    for r in rng.integers(0, A.shape[0], size=40):
        A.rows[r], A.data[r] = [], []
    for r in range(640, 704):
        A.rows[r], A.data[r] = [], []
    A = A.tocsr()
    for r in range(0, A.shape[0], 5):
        lo, hi = A.indptr[r], A.indptr[r + 1]
        k = (hi - lo) // 3
        o = (np.arange(k)[::-1][:, None] * 3 + np.arange(3)[None, :]).ravel()
        A.indices[lo:hi] = A.indices[lo:hi][o]
        A.data[lo:hi] = A.data[lo:hi][o]
    A.has_sorted_indices = False
    return A


DAMAGED_KNOBS = [({}, True), ({'PRCG_SELL_RUNS': '0'}, True), ({'PRCG_SELL_NT': '1'}, True), ({'PRCG_SELL_GRID_PER_CU': '1'}, True),
                 ({'PRCG_SELL_WINDOW': '0'}, False), ({'PRCG_SELL_SIGMA': '256'}, False),
                 ({'PRCG_SELL_WINDOW': '24', 'PRCG_SELL_SIGMA': '64', 'PRCG_SELL_MAX_OVERHEAD_PCT': '600'}, True)]


@pytest.mark.gpu
@pytest.mark.parametrize('knobs,window', DAMAGED_KNOBS, ids=['default', 'runs0', 'nt1', 'grid_per_cu1', 'window0', 'sigma256', 'window24_cut'])
def test_product_on_damaged_fem(amd, knobs, window):
    """k_sell_win / k_sell_tiles with four vectors under the knob sets of test_sliced_rows_with_window_codes: one code per run
    of three and per nonzero, nontemporal loads, one workgroup per CU asked for, delta codes, sorting windows, cut slices."""
    A = damaged_fem()
    X = four_columns(np.random.default_rng(5), A.shape[0])
    product_bits(amd, A, X, knobs, dict(sliced_rows=True, window_codes=window), knobs)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['block_band_16_pages', 'more_waves_than_slices', 'irregular_window', 'irregular_sorted', 'ragged_special_values',
                                  's3_small', 'lap3d', 'bcsstk14_csr'])
def test_product_on_other_operators(amd, case):
    """The 16-page window, a launch with more waves than slices, irregular rows with window codes and with sorting windows,
    ragged rows with +-0 / inf / nan values and unsorted / duplicate indices, and one operator of each fallback family."""
    P = amd['problems']
    rng = np.random.default_rng(77)
    knobs, equal_nan = {}, False
    if case == 'block_band_16_pages':
        A, knobs, family = P.block_band_3dof(1500, 120), {'PRCG_SELL_SIGMA': '64'}, dict(sliced_rows=True, window_codes=True)
    elif case == 'more_waves_than_slices':
        A, family = P.fem_like_3d(6, 3), dict(sliced_rows=True, window_codes=True)
    elif case == 'irregular_window':
        A, family = P.fem_irregular_3d(12), dict(sliced_rows=True, window_codes=True, sorted_windows=False)
    elif case == 'irregular_sorted':
        A, knobs, family = P.fem_irregular_3d(12), {'PRCG_SELL_WINDOW': '0'}, dict(sliced_rows=True, window_codes=False, sorted_windows=True)
    elif case == 'ragged_special_values':           # trial 1 of test_sliced_row_kernels_on_randomised_medium_rows
        n = 7919
        lens = rng.integers(100, 126, size=n)
        lens[rng.integers(0, n, size=n // 100)] = 0
        indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
        rows = np.repeat(np.arange(n), lens)
        cols = np.clip(rows + rng.integers(-2000, 2001, size=rows.size), 0, n - 1).astype(np.int32)
        vals = rng.standard_normal(rows.size)
        vals[rng.integers(0, vals.size, size=50)] = 0.0
        vals[rng.integers(0, vals.size, size=50)] = -0.0
        vals[rng.integers(0, vals.size, size=5)] = np.inf
        vals[rng.integers(0, vals.size, size=5)] = np.nan
        A = sp.csr_matrix((vals, cols, indptr), shape=(n, n))
        A.has_canonical_format = False
        family, equal_nan = dict(sliced_rows=True, window=False), True
    else:
        (A, family), knobs = operator(case), KNOBS.get(case, {})
    X = four_columns(rng, A.shape[0])
    product_bits(amd, A, X, knobs, family, case, equal_nan=equal_nan)


# ---- 2. more than one slice per wave --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fem48():
    from new_cg_variants_amd import problems as P
    A = P.fem_like_3d(48)
    assert A.shape[0] == 331776
    return A


@pytest.mark.gpu
@pytest.mark.parametrize('window', ['1', '0'])
def test_product_with_several_slices_per_wave(amd, window):
    """fem_like_3d(48): 5184 slices for at most 1024 (window codes: one workgroup per CU) or 2048 resident waves -- the
    slice-to-slice pipeline (pages and granule starts one and two slices ahead, the trip carried across the boundary)."""
    A = fem48()
    X = four_columns(np.random.default_rng(3), A.shape[0])
    op = amd['device'].DeviceCSR(A, knobs={'PRCG_SELL_WINDOW': window})
    try:
        s = op.schedule()
        assert s['sliced_rows'] and s['window_codes'] == (window == '1'), s
        Y, _ = op.matmat4(X)
    finally:
        op.close()
    for c in range(4):
        assert np.array_equal(Y[:, c], A @ X[:, c]), (window, c)


@pytest.mark.gpu
def test_session_with_several_slices_per_wave(amd):
    """... and 3 iterations of a four-RHS Hestenes-Stiefel session with Jacobi on it, against the oracle"""
    L = amd['L']
    A = fem48()
    n = A.shape[0]
    B, X0, iters = four_rhs(A), np.zeros((4, n)), 3
    op = amd['device'].DeviceCSR(A)
    try:
        got, sched = device_columns(op, L, 'hs', B, X0, iters, 1 / A.diagonal(), chunks=(2,))
    finally:
        op.close()
    assert sched['rhs4'] and sched['spmm4'] and not sched['rhs2'], sched
    for j in range(4):
        want = oracle_column(A, B[j], X0[j], iters, True, 'hs')
        check_finite(want, 'hs', f'fem48 column {j}')
        assert_column_bits(got[j], want, 'hs', f'fem48 column {j}')


# ---- 3. sessions against the device-ordered oracle ------------------------------------------------------------------------
def _iters(variant, name, jacobi):
    if (name, jacobi) == ('s3_small', True):
        return 40 if variant == 'hs' else 5         # (the counts of the two-RHS tests: the oracle breaks down later)
    return 60


CASES = ([(variant, name, jac, _iters(variant, name, jac), False)
          for variant in ('hs', 'pr', 'm')
          for name in ('fem12', 'fem_irregular10', 'bcsstk14', 's3_small', 'lap3d', 'bcsstk14_csr')
          for jac in (False, True)]
         + [('pr', 'fem12', True, 60, True)])


@pytest.mark.gpu
@pytest.mark.parametrize('variant,name,jacobi,iters,x0_nonzero', CASES)
def test_bits_against_the_device_ordered_oracle(amd, variant, name, jacobi, iters, x0_nonzero):
    """All four columns of a four-RHS session against four oracle runs: every vector, every scalar of every iteration, the
    coefficients, the predicted nu (pr / m) and the history -- equal bits; one four-vector launch on sliced rows, two
    two-vector launches on the window, pattern and CSR-adaptive operators."""
    L = amd['L']
    matrix = 'bcsstk14' if name == 'bcsstk14_csr' else name
    A, B, X0 = problem(matrix, x0_nonzero)
    _, family = operator(name)
    want = [reference(matrix, variant, jacobi, iters, x0_nonzero, j) for j in range(4)]
    for j in range(4):
        check_finite(want[j], variant, f'{variant} {name} jacobi={jacobi} column {j}')
    op = amd['device'].DeviceCSR(A, knobs=KNOBS.get(name))
    try:
        got, sched = device_columns(op, L, variant, B, X0, iters, 1 / A.diagonal() if jacobi else None)
    finally:
        op.close()
    assert sched['rhs4'] and not sched['rhs2'] and not sched['small'] and not sched['fused'], sched
    assert sched['spmm4'] == family['sliced_rows'], sched
    for key, val in family.items():
        assert sched[key] == val, (name, key, sched)
    for j in range(4):
        assert_column_bits(got[j], want[j], variant, f'{variant} {name} jacobi={jacobi} column {j}')


# ---- 4. four = two pairs ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('variant,jacobi', [('hs', True), ('pr', False), ('m', True)])
@pytest.mark.parametrize('name', ['fem12', 'lap3d'])
def test_four_columns_are_two_pairs(amd, name, variant, jacobi):
    """On one handle: a four-RHS session, then two two-RHS sessions begun with columns (0, 1) and (2, 3): every per-column
    output is equal; and the four-RHS session with PRCG_SPMM4=0 gives the same."""
    L = amd['L']
    A, B, X0 = problem(name)
    inv_diag = 1 / A.diagonal() if jacobi else None
    iters = 20
    op = amd['device'].DeviceCSR(A)
    off = amd['device'].DeviceCSR(A, knobs={'PRCG_SPMM4': '0'})
    try:
        four, s4 = device_columns(op, L, variant, B, X0, iters, inv_diag)
        pairs = [device_columns(op, L, variant, B[2 * g:2 * g + 2], X0[2 * g:2 * g + 2], iters, inv_diag) for g in range(2)]
        two, s2 = device_columns(off, L, variant, B, X0, iters, inv_diag)
    finally:
        op.close()
        off.close()
    assert s4['rhs4'] and s4['spmm4'] == s4['sliced_rows'] and s2['rhs4'] and not s2['spmm4'], (s4, s2)
    for g in range(2):
        assert pairs[g][1]['rhs2'] and not pairs[g][1]['rhs4'] and not pairs[g][1]['spmm4'], pairs[g][1]
        for c in range(2):
            assert_columns_equal(four[2 * g + c], pairs[g][0][c], f'{name} {variant}: column {2 * g + c} vs pair {g}')
    for j in range(4):
        assert_columns_equal(two[j], four[j], f'{name} {variant}: PRCG_SPMM4=0, column {j}')


# ---- 5. columns are independent ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['hs', 'pr'])
def test_columns_are_independent(amd, variant):
    """A permutation of the right-hand sides permutes the results, four equal columns give four equal results, and b = 0 in
    column 2 (0 / 0 at once) leaves the other three columns' bits alone while its own history holds the oracle's NaNs."""
    L = amd['L']
    A, B, X0 = problem('fem12')
    n = A.shape[0]
    iters = 25
    Bz = B.copy()
    Bz[2] = 0.0
    op = amd['device'].DeviceCSR(A)
    try:
        base, sched = device_columns(op, L, variant, B, X0, iters, None)
        perm, _ = device_columns(op, L, variant, B[list(PERM)], X0, iters, None)
        equal, _ = device_columns(op, L, variant, np.stack([B[1]] * 4), X0, iters, None)
        zero, _ = device_columns(op, L, variant, Bz, X0, iters, None)
    finally:
        op.close()
    assert sched['rhs4'] and sched['spmm4'], sched
    for j, src in enumerate(PERM):
        assert_columns_equal(perm[j], base[src], f'{variant}: column {j} of the permuted session vs column {src}')
    for j in range(4):
        assert_columns_equal(equal[j], base[1], f'{variant}: four equal columns, column {j}')
    for j in (0, 1, 3):
        assert_columns_equal(zero[j], base[j], f'{variant}: column {j} beside a column that broke down')
        assert np.isfinite(zero[j]['hist']).all()
    want = reference('fem12', variant, False, iters, False, 'zero')
    assert want['hist'][0] == 0.0 and np.isnan(want['hist'][1:]).all()
    assert same(zero[2]['hist'], want['hist'])
    assert_column_bits(zero[2], want, variant, f'{variant}: the column that broke down')


# ---- 6. nothing else moved --------------------------------------------------------------------------------------------------
def single_pr(op, L, b, x0, iters):
    return single_session(op, L, L.PR, b, x0, iters)


def assert_single_equal(run, first, what):
    assert run[0] == first[0], (what, run[0], first[0])
    for v in VECS:
        assert same(run[1][v], first[1][v]), (what, v)
    assert same(run[2], first[2]) and same(run[3], first[3]) and same(run[4], first[4]), what


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['fem12', 's3_small'])
def test_nothing_else_moved(amd, name):
    """On one handle: a single pr session, a two-RHS session, a four-RHS session, the two-RHS session again, the single one
    again -- each repeated run equals its first and a fresh handle's; rhs2 / rhs4 / spmm4 are set as defined."""
    L = amd['L']
    A, B, X0 = problem(name)
    n = A.shape[0]
    iters = 12
    op = amd['device'].DeviceCSR(A)
    fresh = amd['device'].DeviceCSR(A)
    try:
        single1 = single_pr(op, L, B[0], X0[0], iters)
        two1, s2 = device_columns(op, L, 'pr', B[:2], X0[:2], iters, None)
        _, s4 = device_columns(op, L, 'pr', B, X0, iters, 1 / A.diagonal())
        two2, s2b = device_columns(op, L, 'pr', B[:2], X0[:2], iters, None)
        single2 = single_pr(op, L, B[0], X0[0], iters)
        two_fresh, s2f = device_columns(fresh, L, 'pr', B[:2], X0[:2], iters, None)
        single_fresh = single_pr(fresh, L, B[0], X0[0], iters)
    finally:
        op.close()
        fresh.close()
    assert s4['rhs4'] and not s4['rhs2'] and s4['spmm4'] == s4['sliced_rows'], s4
    for s in (s2, s2b, s2f):
        assert s['rhs2'] and not s['rhs4'] and not s['spmm4'], s
    assert s2 == s2b == s2f
    for s in (single1[0], single2[0], single_fresh[0]):
        assert not s['rhs2'] and not s['rhs4'] and not s['spmm4'], s
    assert_single_equal(single2, single1, 'single session after the multi-RHS sessions')
    assert_single_equal(single_fresh, single1, 'single session on a fresh handle')
    for j in range(2):
        assert_columns_equal(two2[j], two1[j], f'two-RHS session after a four-RHS session, column {j}')
        assert_columns_equal(two_fresh[j], two1[j], f'two-RHS session on a fresh handle, column {j}')


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(amd):
    """nrhs 3 and 5, j = 4, the single-column accessors inside a four-RHS session, and every condition the two-RHS session
    refuses -- with the two-RHS session's texts; the session is intact after a refusal."""
    L, cgv = amd['L'], amd['cgv']
    A, B, X0 = problem('fem12')
    n = A.shape[0]
    lib = L.lib()
    op = amd['device'].DeviceCSR(A)
    try:
        with _raises(L, 'PRCG_HS'):
            op.begin_multi(L.PIPE_PR, B, X0, 8)
        with _raises(L, 'history bits other than PRCG_HIST_UPDATED_RESIDUAL_2_NORM'):
            op.begin_multi(L.HS, B, X0, 8, hist_mask=L.HIST_RESIDUAL_2_NORM)
        for nrhs in (3, 5):
            ptrs = (C.c_void_p * nrhs)(*[B[j % 4].ctypes.data for j in range(nrhs)])
            rc = lib.prcg_solve_begin_multi(op._h, L.HS, nrhs, ptrs, ptrs, 8, None, 0)
            assert rc == L.EINVAL and b'nrhs = %d' % nrhs in lib.prcg_last_error(op._h)
        op.begin(L.HS, B[0], X0[0], 4, preconditioner=lambda v: 0.5 * v[::-1][::-1] + 0.0)
        with _raises(L, 'host-callback preconditioner'):
            op.begin_multi(L.HS, B, X0, 8)
        bj = cgv.BlockJacobi(A, 3)
        op.begin(L.HS, B[0], X0[0], 4, block_jacobi=(3, bj.inv_blocks))
        with _raises(L, 'block-Jacobi preconditioner'):
            op.begin_multi(L.HS, B, X0, 8)
        op.clear_preconditioners()
        op.set_replace_hook(lambda k: False)
        with _raises(L, 'replace hook'):
            op.begin_multi(L.HS, B, X0, 8)
        op.set_replace_hook(None)
        op.begin(L.HS, B[0], X0[0], 4)
        with _raises(L, 'no open two-RHS session'):
            op.get_vector('x', rhs=3)
        op.begin_multi(L.HS, B, X0, 8, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM)
        op.iterate(2)
        for call in (lambda: op.get_vector('x'), lambda: op.set_vector('x', B[0]), lambda: op.get_scalars(1),
                     lambda: op.set_scalars(1, np.zeros(L.NUM_SCALARS)), lambda: op.get_coefficients(1),
                     lambda: op.history(), lambda: op.set_iteration(1)):
            with _raises(L, 'two right-hand sides'):
                call()
        for call in (lambda: op.get_vector('x', rhs=4), lambda: op.get_scalars(1, rhs=4), lambda: op.get_coefficients(1, rhs=4),
                     lambda: op.history(rhs=4), lambda: op.get_vector('x', rhs=-1)):
            with _raises(L, 'right-hand side -?[14] out of range'):
                call()
        with _raises(L, 'not part of the two-RHS session'):
            op.get_vector('rt', rhs=3)           # no Jacobi in this session
        with _raises(L, 'not part of the two-RHS session'):
            op.get_vector('st', rhs=2)
        # a refused begin leaves the open session as it was
        with _raises(L, 'PRCG_HS'):
            op.begin_multi(L.PIPE_PR, B, X0, 8)
        op.iterate(1)
        op.sync()
        assert op.k == 3 and op.schedule()['rhs4'] and all(np.isfinite(op.get_vector('x', rhs=j)).all() for j in range(4))
        # inside a two-RHS session the answer for j = 2 is what it was
        op.begin_multi(L.HS, B[:2], X0[:2], 8)
        with _raises(L, 'right-hand side 2 out of range'):
            op.get_vector('x', rhs=2)
    finally:
        op.close()
    ghost = amd['device'].DeviceCSR(sp.hstack([A, sp.csr_matrix((n, 5))]).tocsr())
    try:
        with _raises(L, 'n_ghost = 5 > 0'):
            ghost.begin_multi(L.HS, B, X0, 8)
    finally:
        ghost.close()


@pytest.mark.gpu
def test_refused_with_a_communicator(amd):
    from test_distributed import rccl_ids
    L = amd['L']
    A, B, X0 = problem('fem12')
    uid, path = rccl_ids(1)
    comm = amd['device'].DeviceCSR(A, comm_init=(0, 1, uid, path))
    try:
        with _raises(L, 'communicator'):
            comm.begin_multi(L.HS, B, X0, 8)
    finally:
        comm.close()


# ---- 8. Python shape --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_multi_functions_return_four_trials(amd):
    """hs_pcg_multi / pr_pcg_multi with (4, n) arrays: four trial dicts, the histories the oracle's, light host callbacks
    called per column in column order."""
    cgv, cbs = amd['cgv'], amd['cbs']
    A, B, X0 = problem('fem12')
    iters = 30
    seen = []

    def light(**env):
        seen.append((env['output']['rhs'], env['k']))
    light.prcg_host_light = True
    hs = cgv.hs_pcg_multi(A, B, X0, iters + 1, preconditioner=cgv.Jacobi(A), callbacks=[cbs.updated_residual_2_norm, light])
    pr = cgv.pr_pcg_multi(A, B, X0, iters + 1, preconditioner=cgv.Jacobi(A), callbacks=[cbs.updated_residual_2_norm])
    cgv.clear_operator_cache()
    assert seen == [(j, k) for k in range(iters + 1) for j in range(4)]
    assert len(hs) == 4 and len(pr) == 4
    for j in range(4):
        assert hs[j]['name'] == 'hs_pcg_multi' and hs[j]['rhs'] == j and hs[j]['max_iter'] == iters + 1 and pr[j]['name'] == 'pr_pcg_multi'
        assert same(hs[j]['updated_residual_2_norm'], reference('fem12', 'hs', True, iters, False, j)['hist']), j
        assert same(pr[j]['updated_residual_2_norm'], reference('fem12', 'pr', True, iters, False, j)['hist']), j
