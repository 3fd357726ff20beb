"""Each column of a PIPELINED two-RHS session stopped at its own residual threshold, decided on the device (prcg.h:
prcg_set_stop_rhs / prcg_get_stops_rhs; DeviceCSR.begin_multi_pipe(rr_stop=...), stops_rhs(); rtol= / atol= of
cg_variants.pipe_pr_cg_multi / pipe_pr_pcg_multi / pipe_pr_m_cg_multi / pipe_pr_m_pcg_multi).

The rule is prcg_set_stop's on the column's own row of scalars; a stopped column keeps the complete state of its stop iteration
while the other runs on with the bits it carries in a session without thresholds.  Everything is compared bit for bit with the
device-ordered oracle of tests/test_multi_rhs_pipe.py (no tolerance anywhere; NaN equals NaN).  Thresholds come from the oracle
alone: rr of one of its rows; where the oracle's rule then fires FIRST is where the device must stop (r.r is not monotone).
The harness: tests/multi_rhs_stop_common.py.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import test_multi_rhs_pipe as pipe
from multi_rhs_common import KNOBS, _raises, amd, same, single_session      # noqa: F401  (amd: the fixture)
from multi_rhs_stop_common import ITERS, assert_equal_columns, case, frozen, read, reference, session, stop_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = pipe.NAMES
CONVERGED, BREAKDOWN = 1, 2

# The oracle's table (device_dot, 60 iterations, the right-hand sides of two_rhs, x0 = 0): (operator, Jacobi, flavour, i, j) -> where
# the rule first fires under thr_0 = rr of column 0's row i, thr_1 = rr of column 1's row j.  test_the_oracle_gives_the_table (no
# GPU) restates it; the GPU cases derive their expectations from the oracle again and assert the table's preconditions first.
TABLE = {}
for _fl in ('pr', 'pr_m'):
    for _jac in (False, True):
        TABLE[('lap3d', _jac, _fl, 20, 45)] = (20, 45)       # window, pattern tiles: two two-vector products
        TABLE[('lap3d', _jac, _fl, 45, 20)] = (45, 20)       # ... column 1 freezes first
    TABLE[('fem12', True, _fl, 20, 45)] = (20, 45)           # sliced rows: the one-launch four-vector product
    TABLE[('fem12', False, _fl, 20, 45)] = (20, 43)
TABLE[('fem_irregular10', True, 'pr', 20, 45)] = (20, 45)    # sliced rows of varying length
TABLE[('bcsstk14', True, 'pr', 20, 45)] = (18, 41)           # sliced rows; and (bcsstk14_csr) the CSR-adaptive tiles
STOP_CASES = [(name, jac, fl, i, j) for (name, jac, fl, i, j) in TABLE] + [('bcsstk14_csr', True, 'pr', 20, 45)]


def matrix_of(name):
    return 'bcsstk14' if name == 'bcsstk14_csr' else name          # the same matrix, another product family: one oracle run


def case_id(c):
    return '-'.join(str(q) for q in c)


def thresholds_of(name, jacobi, flavour, i, j, iters=ITERS):
    """multi_rhs_stop_common.case with the preconditions every GPU case asserts before it touches the device"""
    thr, stops = case(matrix_of(name), flavour, jacobi, i, j, iters)
    live = [c for c, q in enumerate((i, j)) if q is not None]
    for c in live:
        assert 0 < stops[c][0] < iters - 1 and stops[c][1] == CONVERGED, (name, c, stops)
    if len(live) == 2:
        assert stops[0][0] != stops[1][0], stops
    return thr, stops


# ---- no GPU needed --------------------------------------------------------------------------------------------------------
def test_header_and_binding():
    """Both entries are declared, exported and bound; prcg_version stays 1; the new header section states the rule."""
    from new_cg_variants_amd import _lib as L, device
    text = open(os.path.join(ROOT, 'include', 'prcg.h')).read()
    pub = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = L.lib()
    assert re.search(r'\bint\s+prcg_set_stop_rhs\s*\(\s*prcg_t\s*\*\s*h\s*,\s*int\s+nrhs\s*,\s*const\s+double\s*\*\s*rr_stop\s*\)', pub)
    assert re.search(r'\bint\s+prcg_get_stops_rhs\s*\(\s*prcg_t\s*\*\s*h\s*,\s*int32_t\s*\*\s*k_stop\s*,\s*int32_t\s*\*\s*status\s*\)', pub)
    for name in ('prcg_set_stop_rhs', 'prcg_get_stops_rhs'):
        assert name in L._SIGNATURES and hasattr(lib, name), name
    assert lib.prcg_version() == 1
    section = text[text.index('each column of a PIPELINED TWO-RHS session stopped at its own residual threshold'):
                   text.index('a BATCH of small independent systems')]
    for word in ('prcg_set_stop_rhs', 'prcg_get_stops_rhs', 'rr <= rr_stop[c]', '!(0 < mu && mu < inf && 0 < nu && nu < inf)', 'converged',
                 'breakdown', 'NULL clears', 'nrhs', 'must be 2', 'prcg_solve_begin_multi_pipe', 'prcg_solve_begin_multi_block_jacobi',
                 'prcg_set_stop_rhs(h, 0, NULL)', 'max(k_0, k_1)', 'read as zero', 'bit for bit'):
        assert word in section, word
    assert 'ignore the threshold' in text                # (prcg_set_stop's own sentence stays)
    assert inspect.signature(device.DeviceCSR.begin_multi_pipe).parameters['rr_stop'].default is None
    assert callable(device.DeviceCSR.stops_rhs)


def test_python_argument_checks_come_before_any_device_call(monkeypatch):
    """rtol= / atol= of the four pipelined functions: wrong shapes, NaN, inf and negative values are ValueErrors naming the
    function, the keyword and the system, raised before an operator is uploaded; the other *_multi functions pass the keywords by."""
    import new_cg_variants_amd.callbacks as cbs
    import new_cg_variants_amd.cg_variants as cgv
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
        for key in ('rtol', 'atol'):
            with pytest.raises(ValueError, match=rf'{name}: {key} must be one value or 2 values, one per system -- got shape \(3,\)'):
                f(A, B, X0, 5, **{key: [1e-8, 1e-8, 1e-8]})
            with pytest.raises(ValueError, match=rf'{name}: {key} must be one value or 2 values, one per system -- got shape \(1, 2\)'):
                f(A, B, X0, 5, **{key: [[1e-8, 1e-8]]})
            with pytest.raises(ValueError, match=rf'{name}: {key}\[0\] = nan: the value of system 0 must be finite and >= 0'):
                f(A, B, X0, 5, **{key: np.nan})
            with pytest.raises(ValueError, match=rf'{name}: {key}\[1\] = nan: the value of system 1 must be finite and >= 0'):
                f(A, B, X0, 5, **{key: [0.0, np.nan]})
            with pytest.raises(ValueError, match=rf'{name}: {key}\[1\] = inf'):
                f(A, B, X0, 5, **{key: [1e-8, np.inf]})
            with pytest.raises(ValueError, match=rf'{name}: {key}\[0\] = -1.0'):
                f(A, B, X0, 5, **{key: -1.0})
        # the shapes of B and X0 are still checked first
        with pytest.raises(ValueError, match=r'%s: .* shape \(2, %d\)' % (name, n)):
            f(A, np.ones(n), X0, 5, rtol=1e-8)
        # what IS served gets as far as the device: either keyword, both, one value or one per system, zero
        for kw in (dict(rtol=1e-8), dict(atol=[1e-3, 1e-5]), dict(rtol=[1e-8, 0.0], atol=1e-12), dict(rtol=0.0)):
            with pytest.raises(AssertionError, match='the device was reached'):
                f(A, B, X0, 5, callbacks=[cbs.updated_residual_2_norm], **kw)
    for name in ('pipe_pr_pcg_multi', 'pipe_pr_m_pcg_multi'):
        with pytest.raises(AssertionError, match='the device was reached'):
            getattr(cgv, name)(A, B, X0, 5, preconditioner=cgv.Jacobi(A), rtol=1e-8)
        with pytest.raises(ValueError, match='block-Jacobi'):           # refused as ever, keywords or not
            getattr(cgv, name)(A, B, X0, 5, preconditioner=cgv.BlockJacobi(A, 3), rtol=1e-8)
    # the multi-RHS functions that cannot stop never took the keywords and pass them by like any keyword they do not know
    for name in ('hs_cg_multi', 'hs_pcg_multi', 'pr_cg_multi', 'pr_pcg_multi', 'm_cg_multi', 'm_pcg_multi'):
        with pytest.raises(AssertionError, match='the device was reached'):
            getattr(cgv, name)(A, B, X0, 5, rtol=-1.0)
    with pytest.raises(AssertionError, match='the device was reached'):
        cgv.hs_bpcg_multi(A, B, X0, 5, preconditioner=cgv.BlockJacobi(A, 3), rtol=-1.0)
    # DeviceCSR.begin_multi_pipe: two thresholds, finite and >= 0, checked before the library is called
    bare = object.__new__(device.DeviceCSR)
    bare.n, bare._lib, bare._h = n, None, None
    for bad, text in (([1.0], r'rr_stop must be one value or 2 values'), ([1.0, 2.0, 3.0], r'got shape \(3,\)'),
                      ([1.0, np.nan], r'rr_stop\[1\] = nan'), ([-1.0, 1.0], r'rr_stop\[0\] = -1.0'), ([np.inf, 1.0], r'rr_stop\[0\] = inf')):
        with pytest.raises(ValueError, match=text):
            bare.begin_multi_pipe(L.PIPE_PR, B, X0, 5, rr_stop=bad)
    # thr_c = max(rtol_c ||b_c||, atol_c)^2: the batches', the single functions' and these come from one place
    thr = cgv._stop_thresholds('f', [1e-3, 1e-2], 1e-9, [B[0], 2 * B[1]])
    assert np.array_equal(thr, np.maximum(np.array([1e-3, 1e-2]) * np.array([np.linalg.norm(B[0]), np.linalg.norm(2 * B[1])]), 1e-9) ** 2)


@pytest.mark.parametrize('name,jacobi,flavour,i,j', list(TABLE), ids=[case_id(c) for c in TABLE])
def test_the_oracle_gives_the_table(name, jacobi, flavour, i, j):
    """The model case: the oracle's rows under device_dot give exactly the (k_0, k_1) the GPU cases rely on, every stop a
    convergence strictly inside the run, and a zero threshold never fires.  A changed harness right-hand side shows up here."""
    thr, stops = thresholds_of(name, jacobi, flavour, i, j)
    assert (stops[0][0], stops[1][0]) == TABLE[(name, jacobi, flavour, i, j)], stops
    for c in range(2):
        rows = reference(name, flavour, jacobi, c)['scalars']
        assert rows.shape == (ITERS + 1, 5) and np.isfinite(rows).all()
        assert thr[c] > 0 and not thr[c] >= rows[0, 4], 'a threshold below the initial r.r: the rule must not fire at k = 0'
        assert stop_of(rows, 0.0) == (-1, 0)


def test_the_oracle_breaks_down_where_the_breakdown_case_says():
    """s3_small under Jacobi, pipe_pr_m_pcg: mu or nu leaves (0, inf) at k = 6 in both columns, with r.r far above 1e-300 before"""
    for c in range(2):
        rows = reference('s3_small', 'pr_m', True, c)['scalars']
        assert stop_of(rows, 1e-300) == (6, BREAKDOWN), c
        assert (rows[:7, 4] > 1e-300).all() and np.isfinite(rows[:6]).all()


@pytest.mark.parametrize('n', [63, 257, 513, 2049])
@pytest.mark.parametrize('jacobi', [False, True])
def test_the_oracle_stops_the_tridiagonal_cases_inside_their_run(n, jacobi):
    thr, stops = size_case(n, jacobi)
    assert 0 < stops[0][0] < 19 and stops[0][1] == CONVERGED and stops[1] == (-1, 0), stops


SIZE_ITERS = 20


def size_case(n, jacobi):
    """tridiag<n>, 20 iterations: thr_0 = rr of column 0's row 5 -- or of the first later row -- under which the oracle stops
    column 0 in (0, 19); thr_1 = 0"""
    for i in range(5, SIZE_ITERS - 1):
        thr, stops = case(f'tridiag{n}', 'pr', jacobi, i, None, SIZE_ITERS)
        if 0 < stops[0][0] < SIZE_ITERS - 1:
            return thr, stops
    raise AssertionError(f'tridiag{n}: no row of the oracle run stops column 0 inside the run')


# ---- 1. each column stops where the oracle does -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name,jacobi,flavour,i,j', STOP_CASES, ids=[case_id(c) for c in STOP_CASES])
def test_each_column_stops_where_the_oracle_does(amd, name, jacobi, flavour, i, j):
    """Three sessions on one handle: (i) no thresholds -- the existing 60-iteration reference; (ii) thresholds, ONE call of 59
    iterations, prcg_sync, three more iterations that change nothing; (iii) thresholds, calls cut at k_first, k_first + 1 and
    k_second.  A stopped column holds the oracle's state of its stop iteration, every later row zero; up to the first stop both
    columns equal session (i) row by row."""
    L = amd['L']
    matrix = matrix_of(name)
    A, B, X0 = pipe.problem(matrix)
    thr, stops = thresholds_of(name, jacobi, flavour, i, j)
    (k0, _), (k1, _) = stops
    k_first, k_second = min(k0, k1), max(k0, k1)
    first = 0 if k0 < k1 else 1
    want = [frozen(matrix, flavour, jacobi, c, stops[c][0]) for c in range(2)]
    full = [reference(matrix, flavour, jacobi, c) for c in range(2)]
    variant = pipe.variant_of(L, flavour)
    inv_diag = 1 / A.diagonal() if jacobi else None
    seen = []
    op = amd['device'].DeviceCSR(A, knobs=KNOBS.get(name))
    try:
        plain, sched = pipe.device_columns(op, L, variant, B, X0, ITERS, inv_diag)
        plain_stops = op.stops_rhs()
        one = session(op, L, variant, B, X0, ITERS, inv_diag, thr, (ITERS - 1,))
        op.iterate(3)                              # both columns have stopped: a no-op
        op.sync()
        again = read(op, L, ITERS, jacobi)
        cut = session(op, L, variant, B, X0, ITERS, inv_diag, thr, (k_first, 1, k_second - k_first - 1),
                      after=lambda _: seen.append((op.stops_rhs(), op.k)))
        op.iterate(3)
        op.sync()
        cut_again = (op.stops_rhs(), op.k)
    finally:
        op.close()
    what = f'{name} jacobi={jacobi} {flavour} thresholds from rows ({i}, {j})'
    assert sched['rhs2_pipe'] and sched['spmm4'] == pipe.SPMM4[name], sched
    # (i) the session without thresholds is the one it always was, and reports no stop
    assert plain_stops == [(-1, 0), (-1, 0)]
    for c in range(2):
        pipe.assert_column_bits(plain[c], full[c], f'{what}: no thresholds, column {c}')
    # (ii), (iii): the stops, the iteration count, every key of both columns
    for cols, got_stops, k in (one, again, cut):
        assert got_stops == [(k0, CONVERGED), (k1, CONVERGED)], (what, got_stops)
        assert k == k_second, (what, k)
        for c in range(2):
            pipe.assert_column_bits(cols[c], want[c], f'{what}: column {c} stopped at {stops[c][0]}')
            assert not cols[c]['all_scalars'][stops[c][0] + 1:].any(), 'rows beyond the stop read as zero'
            # up to the first stop both columns equal the session without thresholds row by row
            assert same(cols[c]['all_scalars'][:k_first + 1], plain[c]['all_scalars'][:k_first + 1]), (what, c)
            for q in ('alpha', 'beta', 'nu_pred'):
                assert same(cols[c][q][:k_first], plain[c][q][:k_first]), (what, c, q)
    for c in range(2):
        assert_equal_columns(again[0][c], one[0][c], f'{what}: three more iterations change nothing, column {c}')
    # (iii) what the host saw between the calls: one column frozen while the other still runs, then both
    running = [(-1, 0), (-1, 0)]
    one_stopped = list(running)
    one_stopped[first] = (k_first, CONVERGED)
    assert seen[0] == (one_stopped, k_first), seen
    assert seen[1] == (one_stopped, k_first + 1), seen            # a column still runs: the count is what was launched
    assert seen[2] == ([(k0, CONVERGED), (k1, CONVERGED)], k_second), seen
    assert cut_again == seen[2]
    print(f'{what}: stops {stops}, both columns bit-exact in three sessions; schedule {sched}')


# ---- 2. the running column is untouched by its partner's freeze ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name', ['lap3d', 'fem12'])
def test_the_running_column_is_untouched_by_its_partner_freeze(amd, name):
    """thr = (rr of column 0's row 20, 0): column 0 stops at 20, column 1 after 60 iterations equals the session without
    thresholds in every key.  The same with the columns exchanged; and with the right-hand sides exchanged together with the
    thresholds the results exchange bit for bit."""
    L = amd['L']
    A, B, X0 = pipe.problem(name)
    inv_diag = 1 / A.diagonal()
    thr_a, stops_a = thresholds_of(name, True, 'pr', 20, None)
    thr_b, stops_b = thresholds_of(name, True, 'pr', None, 20)
    assert stops_a[0][0] == 20 and stops_a[1] == (-1, 0) and stops_b[0] == (-1, 0)
    op = amd['device'].DeviceCSR(A)
    try:
        plain, sched = pipe.device_columns(op, L, L.PIPE_PR, B, X0, ITERS, inv_diag)
        a = session(op, L, L.PIPE_PR, B, X0, ITERS, inv_diag, thr_a, (7, ITERS - 7))
        b = session(op, L, L.PIPE_PR, B, X0, ITERS, inv_diag, thr_b, (ITERS,))
        a_swapped = session(op, L, L.PIPE_PR, B[::-1], X0[::-1], ITERS, inv_diag, thr_a[::-1], (7, ITERS - 7))
    finally:
        op.close()
    assert sched['spmm4'] == pipe.SPMM4[name]
    for (cols, got_stops, k), stops, stopped in ((a, stops_a, 0), (b, stops_b, 1)):
        assert got_stops == [tuple(s) for s in stops] and k == ITERS, (name, got_stops, k)      # a column still runs: k counts the launches
        assert_equal_columns(cols[1 - stopped], plain[1 - stopped], f'{name}: column {1 - stopped} beside a frozen partner')
        pipe.assert_column_bits(cols[stopped], frozen(name, 'pr', True, stopped, stops[stopped][0]), f'{name}: the frozen column {stopped}')
    assert a_swapped[1] == a[1][::-1] and a_swapped[2] == a[2]
    for c in range(2):
        assert_equal_columns(a_swapped[0][c], a[0][1 - c], f'{name}: exchanged right-hand sides and thresholds, column {c}')


# ---- 3. zero thresholds never fire ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('jacobi', [False, True])
@pytest.mark.parametrize('name', ['lap3d', 'fem12'])
def test_zero_thresholds_never_fire(amd, name, jacobi):
    """Both thresholds 0: the kernels of the stopping session, no stop -- every key equals the session without thresholds."""
    L = amd['L']
    A, B, X0 = pipe.problem(name)
    inv_diag = 1 / A.diagonal() if jacobi else None
    for c in range(2):
        assert stop_of(reference(name, 'pr', jacobi, c)['scalars'], 0.0) == (-1, 0)
    op = amd['device'].DeviceCSR(A)
    try:
        plain, _ = pipe.device_columns(op, L, L.PIPE_PR, B, X0, ITERS, inv_diag)
        cols, got_stops, k = session(op, L, L.PIPE_PR, B, X0, ITERS, inv_diag, [0.0, 0.0], (1, 2, ITERS - 3))
    finally:
        op.close()
    assert got_stops == [(-1, 0), (-1, 0)] and k == ITERS
    for c in range(2):
        assert_equal_columns(cols[c], plain[c], f'{name} jacobi={jacobi}: zero thresholds, column {c}')
        pipe.assert_column_bits(cols[c], reference(name, 'pr', jacobi, c), f'{name} jacobi={jacobi}: column {c} vs the oracle')


# ---- 4. a zero column stops before the first iteration -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('jacobi', [False, True])
@pytest.mark.parametrize('name', ['lap3d', 'fem12'])
def test_a_zero_column_stops_before_the_first_iteration(amd, name, jacobi):
    """B[0] = 0, X0[0] = 0, thresholds 0: column 0 is stopped at 0 as converged (r.r = 0 <= 0) and no row beyond 0 is written;
    column 1 holds its ordinary run."""
    L = amd['L']
    A, B, X0 = pipe.problem(name)
    n = A.shape[0]
    inv_diag = 1 / A.diagonal() if jacobi else None
    zero = reference(name, 'pr', jacobi, 'zero')
    assert stop_of(zero['scalars'], 0.0) == (0, CONVERGED) and np.isnan(zero['hist'][1:]).all()
    op = amd['device'].DeviceCSR(A)
    try:
        cols, got_stops, k = session(op, L, L.PIPE_PR, np.stack([np.zeros(n), B[1]]), X0, ITERS, inv_diag, [0.0, 0.0], (ITERS,))
    finally:
        op.close()
    assert got_stops == [(0, CONVERGED), (-1, 0)] and k == ITERS
    pipe.assert_column_bits(cols[0], frozen(name, 'pr', jacobi, 'zero', 0), f'{name} jacobi={jacobi}: the zero column')
    assert not cols[0]['all_scalars'][1:].any() and not cols[0]['hist'].any() and not cols[0]['x'].any()
    pipe.assert_column_bits(cols[1], reference(name, 'pr', jacobi, 1), f'{name} jacobi={jacobi}: the column beside it')


# ---- 5. a breakdown stops a column -------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_breakdown_stops_a_column(amd):
    """s3_small under Jacobi, pipe_pr_m_pcg: thresholds of 1e-300 are never reached, mu or nu leaves (0, inf) at k = 6 in both
    columns -- status 2, the state of iteration 6, finite x."""
    L = amd['L']
    A, B, X0 = pipe.problem('s3_small')
    for c in range(2):
        assert stop_of(reference('s3_small', 'pr_m', True, c)['scalars'], 1e-300) == (6, BREAKDOWN)
    op = amd['device'].DeviceCSR(A)
    try:
        cols, got_stops, k = session(op, L, L.PIPE_PR_M, B, X0, ITERS, 1 / A.diagonal(), [1e-300, 1e-300], (ITERS - 1,))
    finally:
        op.close()
    assert got_stops == [(6, BREAKDOWN), (6, BREAKDOWN)] and k == 6
    for c in range(2):
        assert np.isfinite(cols[c]['x']).all()
        pipe.assert_column_bits(cols[c], frozen('s3_small', 'pr_m', True, c, 6), f's3_small: column {c} broken down at 6')


# ---- 6. update-kernel sizes --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('jacobi', [False, True])
@pytest.mark.parametrize('n', [63, 257, 513, 2049])
def test_update_kernel_sizes(amd, n, jacobi):
    """A lane with only its first element, a ragged second half, one block and several, a ragged last block -- with one column
    skipped from its stop on: column 0 frozen where the oracle stops it, column 1 (threshold 0) its ordinary 20 iterations."""
    L = amd['L']
    name = f'tridiag{n}'
    A, B, X0 = pipe.problem(name)
    thr, stops = size_case(n, jacobi)
    assert 0 < stops[0][0] < SIZE_ITERS - 1 and stops[1] == (-1, 0)
    inv_diag = 1 / A.diagonal() if jacobi else None
    op = amd['device'].DeviceCSR(A)
    try:
        cols, got_stops, k = session(op, L, L.PIPE_PR, B, X0, SIZE_ITERS, inv_diag, thr, (2, SIZE_ITERS - 2))
        sched = op.schedule()
    finally:
        op.close()
    assert sched['rhs2_pipe'] and not sched['small'], sched
    assert got_stops == [tuple(stops[0]), (-1, 0)] and k == SIZE_ITERS
    pipe.assert_column_bits(cols[0], frozen(name, 'pr', jacobi, 0, stops[0][0], SIZE_ITERS), f'n={n} jacobi={jacobi}: the frozen column')
    pipe.assert_column_bits(cols[1], reference(name, 'pr', jacobi, 1, SIZE_ITERS), f'n={n} jacobi={jacobi}: the running column')


# ---- 7. refusals and leftovers -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refusals(amd):
    """The C-ABI texts: nrhs != 2; NaN / inf / negative thresholds naming the column, what was set before staying; the sessions
    that cannot stop refuse while thresholds are set; prcg_get_stops_rhs without a session and with null buffers; single sessions
    run unaffected; prcg_get_stop keeps refusing the multi session; after clearing every entry is served again."""
    L, cgv = amd['L'], amd['cgv']
    A, B, X0 = pipe.problem('fem12')
    n = A.shape[0]
    d = 1 / A.diagonal()
    lib = L.lib()
    op = amd['device'].DeviceCSR(A)

    def set_stop(nrhs, values):
        v = None if values is None else np.array(values, dtype=np.float64)
        rc = lib.prcg_set_stop_rhs(op._h, nrhs, L.ptr(v))
        return rc, lib.prcg_last_error(op._h).decode()

    def get_stops(k_ok=True, s_ok=True):
        k_stop, status = np.full(4, -7, dtype=np.int32), np.full(4, -7, dtype=np.int32)
        rc = lib.prcg_get_stops_rhs(op._h, L.ptr(k_stop) if k_ok else None, L.ptr(status) if s_ok else None)
        return rc, lib.prcg_last_error(op._h).decode(), k_stop, status

    thr, stops = thresholds_of('fem12', True, 'pr', 20, 45)
    try:
        rc, text, _, _ = get_stops()
        assert rc == L.EINVAL and 'no open multi-RHS session' in text, text
        for nrhs in (1, 3, 4, 0, -2):
            rc, text = set_stop(nrhs, [1.0, 1.0, 1.0, 1.0])
            assert rc == L.EINVAL and f'nrhs = {nrhs}' in text and 'only the pipelined two-RHS session' in text and 'can stop' in text, text
        assert set_stop(2, thr)[0] == L.OK
        for bad, col in (([np.nan, 1.0], 0), ([1.0, np.nan], 1), ([np.inf, 1.0], 0), ([1.0, -np.inf], 1), ([1.0, -1e-300], 1), ([-1.0, 1.0], 0)):
            rc, text = set_stop(2, bad)
            assert rc == L.EINVAL and f'rr_stop[{col}]' in text and f'column {col}' in text and 'finite' in text and '>= 0' in text, text
        # ... what was set before stays: the sessions that cannot stop refuse, the pipelined one stops where the oracle does
        with _raises(L, r'prcg_solve_begin_multi: per-column stop thresholds are set \(prcg_set_stop_rhs\).*pipelined two-RHS session only.*'
                        r'prcg_set_stop_rhs\(h, 0, NULL\) clears'):
            op.begin_multi(L.PR, B, X0, 8, inv_diag=d)
        with _raises(L, r'prcg_solve_begin_multi: per-column stop thresholds are set'):
            op.begin_multi(L.HS, np.vstack([B, B]), np.vstack([X0, X0]), 8)
        bj = cgv.BlockJacobi(A, 3)
        with _raises(L, r'prcg_solve_begin_multi_block_jacobi: per-column stop thresholds are set.*prcg_set_stop_rhs\(h, 0, NULL\) clears'):
            op.begin_multi_block_jacobi(L.PR, B, X0, 8, block_jacobi=(3, bj.inv_blocks))
        op.clear_preconditioners()
        # a single session runs unaffected while these thresholds are set, and its own stop is not theirs
        sched, vec, sc_, cf, hist = single_session(op, L, L.PIPE_PR, B[0], X0[0], 24, d)
        assert not sched['rhs2'] and op.stop() == (-1, 0) and op.k == 24
        rc, text, _, _ = get_stops()
        assert rc == L.EINVAL and 'no open multi-RHS session' in text, text
        # the pipelined session begun through the C entry (signature unchanged) takes the thresholds that were set
        bp, xp = (C.c_void_p * 2)(B[0].ctypes.data, B[1].ctypes.data), (C.c_void_p * 2)(X0[0].ctypes.data, X0[1].ctypes.data)
        assert lib.prcg_solve_begin_multi_pipe(op._h, L.PIPE_PR, 2, bp, xp, ITERS + 1, L.ptr(np.ascontiguousarray(d)), 0) == L.OK
        op.max_iter, op.hist_mask = ITERS + 1, 0
        assert set_stop(2, [0.0, 0.0])[0] == L.OK              # an open session is not affected
        op.iterate(ITERS - 1)
        rc, text, k_stop, status = get_stops()
        assert rc == L.OK and list(k_stop[:2]) == [stops[0][0], stops[1][0]] and list(status[:2]) == [CONVERGED, CONVERGED] and op.k == stops[1][0]
        assert list(k_stop[2:]) == [-7, -7] and list(status[2:]) == [-7, -7], 'nrhs entries each'
        for k_ok, s_ok in ((False, True), (True, False), (False, False)):
            rc, text, _, _ = get_stops(k_ok, s_ok)
            assert rc == L.EINVAL and 'null buffer' in text, text
        with _raises(L, 'two right-hand sides'):
            op.stop()                                            # prcg_get_stop keeps refusing the multi session
        for call in (lambda: op.set_vector('x', B[0]), lambda: op.set_scalars(1, np.zeros(L.NUM_SCALARS)), lambda: op.set_iteration(1)):
            with _raises(L, 'two right-hand sides'):
                call()
        assert same(op.get_vector('x', rhs=0), frozen('fem12', 'pr', True, 0, stops[0][0])['x'])
        # NULL clears, whatever nrhs says: every entry is served again, and the sessions report no stop
        assert set_stop(0, None)[0] == L.OK
        op.begin_multi(L.PR, B, X0, 8, inv_diag=d)
        op.iterate(2)
        assert op.stops_rhs() == [(-1, 0), (-1, 0)]
        op.begin_multi(L.HS, np.vstack([B, B]), np.vstack([X0, X0]), 8)
        op.iterate(2)
        assert op.stops_rhs() == [(-1, 0)] * 4
        op.begin_multi_block_jacobi(L.PR, B, X0, 8, block_jacobi=(3, bj.inv_blocks))
        op.iterate(2)
        assert op.stops_rhs() == [(-1, 0), (-1, 0)]
        op.clear_preconditioners()
        op.begin_multi_pipe(L.PIPE_PR, B, X0, 8, inv_diag=d)
        op.iterate(7)
        assert op.stops_rhs() == [(-1, 0), (-1, 0)] and op.k == 7
        # prcg_set_stop's threshold and these are independent: multi sessions go on ignoring that one
        op.begin(L.PIPE_PR, B[0], X0[0], 30, inv_diag=d, rr_stop=1e300)
        assert op.stop() == (0, CONVERGED)
        one = np.array([1e300])
        assert lib.prcg_set_stop(op._h, L.ptr(one)) == L.OK
        op.begin_multi_pipe(L.PIPE_PR, B, X0, 8, inv_diag=d)
        op.iterate(7)
        assert op.stops_rhs() == [(-1, 0), (-1, 0)] and op.k == 7
        assert lib.prcg_set_stop(op._h, None) == L.OK
        # DeviceCSR.begin_multi_pipe(rr_stop=...) leaves no thresholds behind on the handle
        op.begin_multi_pipe(L.PIPE_PR, B, X0, 8, inv_diag=d, rr_stop=[1e300, 0.0])
        assert op.stops_rhs() == [(0, CONVERGED), (-1, 0)]
        op.begin_multi(L.PR, B, X0, 8, inv_diag=d)
    finally:
        op.close()


@pytest.mark.gpu
@pytest.mark.parametrize('single', ['PIPE_PR', 'HS'])
@pytest.mark.parametrize('name', ['s3_small', 'fem12'])
def test_nothing_left_behind(amd, name, single):
    """On ONE handle: a single session, a pipelined two-RHS session that stops a column (thresholds 1e300 and 0), the same single
    session again.  The single runs are bitwise equal, report the same schedule, and equal a fresh handle's."""
    L = amd['L']
    A, B, X0 = pipe.problem(name)
    n = A.shape[0]
    variant = getattr(L, single)
    vecs = ('x', 'r', 'p', 's')
    iters, multi_iters = 24, 5
    d = 1 / A.diagonal()
    op = amd['device'].DeviceCSR(A)
    fresh = amd['device'].DeviceCSR(A)
    try:
        first = single_session(op, L, variant, B[0], np.zeros(n), iters, vecs=vecs)
        between = session(op, L, L.PIPE_PR, B, X0, multi_iters, d, [1e300, 0.0], (multi_iters,))
        again = single_session(op, L, variant, B[0], np.zeros(n), iters, vecs=vecs)
        other = single_session(fresh, L, variant, B[0], np.zeros(n), iters, vecs=vecs)
    finally:
        op.close()
        fresh.close()
    assert between[1] == [(0, CONVERGED), (-1, 0)] and between[2] == multi_iters
    pipe.assert_column_bits(between[0][1], reference(name, 'pr', True, 1, multi_iters), f'{name}: the session in between, column 1')
    for run, what in ((again, 'after the stopped two-RHS session'), (other, 'fresh handle')):
        assert run[0] == first[0], (what, run[0], first[0])
        for v_ in vecs:
            assert same(run[1][v_], first[1][v_]), (what, v_)
        assert same(run[2], first[2]) and same(run[3], first[3]) and same(run[4], first[4]), what


# ---- 8. the public functions -------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_public_function_stops_each_system(amd):
    """pipe_pr_pcg_multi on fem12 with per-system rtol = sqrt(thr_c) / ||b_c||: 'iterations', 'status' and the histories are those
    of the session of case 1; a light host callback is called k_c + 1 times for column c; a run that ends before its threshold
    reports 'max_iter'."""
    cgv, cbs = amd['cgv'], amd['cbs']
    A, B, X0 = pipe.problem('fem12')
    thr, stops = thresholds_of('fem12', True, 'pr', 20, 45)
    rtol = [np.sqrt(thr[c]) / np.linalg.norm(B[c]) for c in range(2)]
    for c in range(2):                     # (thr_c IS r.r of a row: rounding must not put the function's threshold below it)
        while (rtol[c] * np.linalg.norm(B[c])) ** 2 < thr[c]:
            rtol[c] = np.nextafter(rtol[c], np.inf)
    # the public function squares max(rtol ||b||, atol): the oracle must stop at the same rows under THOSE thresholds
    thr_pub = cgv._stop_thresholds('pipe_pr_pcg_multi', rtol, None, [B[0], B[1]])
    stops_pub = [stop_of(reference('fem12', 'pr', True, c)['scalars'], thr_pub[c]) for c in range(2)]
    assert stops_pub == [tuple(s) for s in stops], (stops_pub, stops)
    calls = {0: [], 1: []}

    def light(output, k, **env):
        calls[output['rhs']].append(k)
    light.prcg_host_light = True
    try:
        trials = cgv.pipe_pr_pcg_multi(A, B, X0, ITERS + 1, preconditioner=cgv.Jacobi(A), callbacks=[cbs.updated_residual_2_norm], rtol=rtol)
        with_light = cgv.pipe_pr_pcg_multi(A, B, X0, ITERS + 1, preconditioner=cgv.Jacobi(A), callbacks=[cbs.updated_residual_2_norm, light],
                                           rtol=rtol)
        short = cgv.pipe_pr_pcg_multi(A, B, X0, 6, preconditioner=cgv.Jacobi(A), callbacks=[cbs.updated_residual_2_norm], rtol=1e-30)
        plain = cgv.pipe_pr_pcg_multi(A, B, X0, ITERS + 1, preconditioner=cgv.Jacobi(A), callbacks=[cbs.updated_residual_2_norm])
    finally:
        cgv.clear_operator_cache()
    for c in range(2):
        want = frozen('fem12', 'pr', True, c, stops[c][0])
        for t in (trials, with_light):
            assert t[c]['name'] == 'pipe_pr_pcg_multi' and t[c]['rhs'] == c and t[c]['max_iter'] == ITERS + 1
            assert t[c]['iterations'] == stops[c][0] and t[c]['status'] == 'converged', (c, t[c]['iterations'], t[c]['status'])
            assert same(t[c]['updated_residual_2_norm'], want['hist']), c
        assert calls[c] == list(range(stops[c][0] + 1)), (c, calls[c])
        assert short[c]['status'] == 'max_iter' and short[c]['iterations'] == 5
        assert same(short[c]['updated_residual_2_norm'], reference('fem12', 'pr', True, c)['hist'][:6])
        assert 'iterations' not in plain[c] and 'status' not in plain[c]
        assert same(plain[c]['updated_residual_2_norm'], reference('fem12', 'pr', True, c)['hist'])
