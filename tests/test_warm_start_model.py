"""CPU: the inputs of tests/test_warm_start.py are valid, and its assertions would notice a faulty start-up.

(1) For every case of that file that can be built without a device (start kinds 'random' and 'solved'; 'restart' needs the
    handle) the oracle -- under np.dot, the batch under the workgroup's sum wg_dot -- has finite, nonzero inner products at every
    iteration of the run's length: the choice of methods, operators and seeds is pinned here.  The GPU tests assert the same again
    under the device's trees, where a breakdown iteration can move.
(2) In the style of tests/test_device_order.py: the oracle started from x0 and from three deliberately FAULTY start-ups -- r0 =
    b + A x0; a product with an x0 whose ghost rows were never exchanged; system s started from system s + 1's vector -- differs
    in the bits of r at k = 0 and of row 0 of the inner products (one exception, stated at its test: there r alone shows the fault).
    Those are the first things the GPU tests compare."""
import numpy as np
import pytest

import small_batch_blocks_common as BB
import small_batch_common as B
import test_trajectory_ranks as TR
import warm_start_common as W
from oracle import ne_oracle as orc
from single_stop_common import CONVERGED, stop_of, trajectory
from trajectory_common import ALL_METHODS, FIELD, run_oracle


@pytest.fixture(scope='module')
def operators(matrices):
    """name -> (A, b, the oracle's Jacobi), built once and left unchanged"""
    cache = {}

    def get(name):
        name = W.MATRIX_OF.get(name, name)
        if name not in cache:
            A, b = W.operator(name, matrices)
            cache[name] = (A, b, orc.jacobi(A))
        return cache[name]
    return get


def inner_products(method, A, b, jacobi, x0, iters, A_start=None):
    """rows of the inner products `method` defines, states 0 .. iters - 1, and the oracle's r at k = 0 (the recorders run against
    x_true = 0 and decide nothing here)"""
    rows, _, snaps = run_oracle(method, A_start if A_start is not None else A, b, np.zeros(A.shape[0]), jacobi, iters, np.dot, np.dot, {0}, x0=x0)
    return rows[:, [FIELD[f] for _, f in ALL_METHODS[method][3]]], snaps[0][1]


def assert_clean(rows, what):
    ok = (np.isfinite(rows) & (rows != 0)).all(axis=1)
    assert rows.shape[0] > 0 and ok.all(), (what, f'the oracle breaks down at k={int(np.argmin(ok))}')


# ---- (1) the inputs are valid ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method,operator', W.SINGLE_CASES, ids=['-'.join(c) for c in W.SINGLE_CASES])
def test_single_sessions_from_the_random_start_do_not_break_down(operators, method, operator):
    A, b, jacobi = operators(operator)
    rows, r0 = inner_products(method, A, b, jacobi, W.random_start(A.shape[0]), W.ITERS)
    assert rows.shape[0] == W.ITERS
    assert_clean(rows, (method, operator))
    assert np.linalg.norm(r0 - b) > np.linalg.norm(b)                # a start far from the solution: A x0 is the larger part of r0


@pytest.mark.parametrize('method,operator,prec', W.STORED_TILDE_CASES, ids=['-'.join(c) for c in W.STORED_TILDE_CASES])
def test_stored_tilde_sessions_from_the_random_start_do_not_break_down(operators, method, operator, prec):
    import new_cg_variants_amd.cg_variants as cgv
    A, b, _ = operators(operator)
    assert prec == 'bs3'
    rows, _ = inner_products(method, A, b, cgv.BlockJacobi(A, 3), W.random_start(A.shape[0]), W.ITERS)
    assert_clean(rows, (method, operator, prec))


@pytest.mark.parametrize('variant,operator', W.SMALL_SOLVER_CASES, ids=['-'.join(c) for c in W.SMALL_SOLVER_CASES])
def test_one_workgroup_sessions_from_the_random_start_do_not_break_down(operators, variant, operator):
    A, b, _ = operators(operator)
    want = B.oracle_stopped(A, b, variant, 0.0, W.ITERS, jacobi=False, x0=W.random_start(A.shape[0]))
    assert want['status'] == 0 and want['last'] == W.ITERS and W.first_bad(want['scalars']) < 0, (variant, operator, want['k_stop'])


@pytest.mark.parametrize('method', ['pipe_pr_cg', 'hs_cg'])
@pytest.mark.parametrize('operator', ['bcsstk03', 'nos7'])
def test_prefix_floor_of_the_random_start_is_one_below_the_references_own_depth(operators, operator, method):
    """W.WARM_PREFIX_FLOOR, measured as tests/test_gpu_parity.py's PREFIX_FLOOR was: the reference's loop from the random start with
    its inner products summed in seven other orders leaves 1e-12 of the BLAS order's recurrence residual at a first k; the floor
    is one iteration below the earliest of them over both methods, and no order parts later than two iterations above it"""
    import math

    from device_order import device_dot, pair_sum
    from test_gpu_parity import first_k_beyond
    A, b, _ = operators(operator)
    x0 = W.random_start(A.shape[0])
    orders = [lambda u, v: float(np.sum(u * v)), lambda u, v: float(np.dot(u[::-1], v[::-1])), device_dot,
              lambda u, v: float(sum(np.dot(u[i::4], v[i::4]) for i in range(4))), lambda u, v: math.fsum(u * v), B.wg_dot,
              lambda u, v: pair_sum(u * v)]

    def history(dot):
        return getattr(orc, method)(A, b, x0, W.ITERS + 1, callbacks=['updated_residual_2_norm'], dot=dot)['updated_residual_2_norm']
    ref = history(np.dot)
    depths = [first_k_beyond(history(dot), ref) for dot in orders]
    floor = W.WARM_PREFIX_FLOOR[operator]
    assert floor + 1 <= min(depths) and max(depths) <= floor + 2, (operator, method, depths)


@pytest.mark.parametrize('operator', W.STOP_OPERATORS)
@pytest.mark.parametrize('method', W.STOP_METHODS)
def test_stopped_sessions_stop_inside_their_run(operators, method, operator):
    """from the random start: the rule with thr = (rtol ||b||)^2 fires at an interior iteration, and not for a breakdown; nothing
    breaks down before it.  From the solved start: r0 is exactly zero and the rule fires at k = 0 with thr = 0."""
    A, b, _ = operators(operator)
    n = A.shape[0]
    x0 = W.random_start(n)
    max_iter, rtol = W.STOP_RUN[(operator, method, 'random')]
    thr = float(B.thresholds([b], rtol=rtol)[0])
    traj = trajectory(A, b, method, np.dot, np.dot, max_iter - 1, keep=(), x0=x0)
    k_stop, status = stop_of(traj, thr)
    assert status == CONVERGED and 0 < k_stop < max_iter - 1, (k_stop, status)
    assert traj['scalars'][0, 4] > 100 * thr and np.isfinite(traj['scalars'][:k_stop + 1]).all()
    assert stop_of(traj, 0.0)[1] == 0 or stop_of(traj, 0.0)[0] > k_stop
    solved = trajectory(A, W.solved_rhs(A, x0), method, np.dot, np.dot, 2, keep=(0,), x0=x0)
    assert not solved['at'][0]['r'].any() and np.array_equal(solved['at'][0]['x'], x0)
    assert stop_of(solved, 0.0) == (0, CONVERGED)
    assert not np.isfinite(solved['scalars'][1]).any()             # without a threshold: 0 / 0 from the first iteration on


def test_the_batch_order_moves_most_systems_to_another_slot(matrices):
    systems = W.batch_systems(matrices)
    assert [name for name, _, _, _ in systems] == [B.NINE[i][0] for i in W.BATCH_ORDER] and sorted(W.BATCH_ORDER) == list(range(9))
    for jacobi in (False, True):
        rc, mode, group = B.plan([B.shape_of(A) for _, A, _, _ in systems], jacobi=jacobi)
        assert rc == 2 and mode.tolist() == [B.NINE[i][2] for i in W.BATCH_ORDER] == [1, 0, 1, 0, 1, 0, 1, 0, 1]
        slot = W.slots_of(mode)
        assert sorted(slot) == list(range(9)) and sum(q != s for s, q in enumerate(slot)) >= 7, slot
    assert W.slots_of([1, 0, 1, 0]) == [0, 2, 1, 3] and W.slots_of([0, 0, 1]) == [1, 2, 0]
    x0s = [x0 for _, _, _, x0 in systems]
    assert all(x0.shape == (A.shape[0],) for (_, A, _, _), x0 in zip(systems, x0s))
    assert len({x0[:48].tobytes() for x0 in x0s}) == 9                # nine different vectors, also on their common rows


@pytest.mark.parametrize('prec', W.BATCH_PRECS)
@pytest.mark.parametrize('variant', B.VARIANTS)
def test_batch_systems_from_their_random_starts(matrices, variant, prec):
    """under the workgroup's sum every system is clean for all ITERS iterations, but the diagonal bcsstm22 under a preconditioner
    (W.BCSSTM22_BREAKS)"""
    for s, (name, A, b, x0) in enumerate(W.batch_systems(matrices)):
        if prec == 'none':
            scalars = B.oracle_stopped(A, b, variant, 0.0, W.ITERS, jacobi=False, x0=x0)['scalars']
            assert scalars.shape[0] == W.ITERS + 1
        else:
            scalars = BB.trajectory(A, b, variant, W.batch_prec(A, s, prec), free=W.ITERS, x0=x0)[0]['scalars']
        want = W.BCSSTM22_BREAKS.get((variant, prec), -1) if name == 'bcsstm22' else -1
        assert W.first_bad(scalars) == want, (name, variant, prec, W.first_bad(scalars))
        assert np.isfinite(scalars[:5]).all() and (scalars[:5, [0, 3, 4]] > 0).all()


@pytest.mark.parametrize('method,operator,nranks,transport', W.RANK_CASES, ids=['-'.join(str(q) for q in c) for c in W.RANK_CASES])
def test_multi_rank_sessions_from_the_random_start_do_not_break_down(method, operator, nranks, transport):
    from new_cg_variants_amd import problems as P
    A = TR.OPERATORS[operator][0](P)
    b = P.reference_rhs(A, A.shape[0])[0]
    rows, _, _ = run_oracle(method, A, b, np.zeros(A.shape[0]), orc.jacobi(A), W.ITERS + 1, np.dot, np.dot, (), x0=W.random_start(A.shape[0]))
    assert rows.shape[0] == W.ITERS + 1 and TR.first_breakdown(rows) < 0, TR.first_breakdown(rows)


# ---- (2) the GPU tests would notice ---------------------------------------------------------------------------------------------
def differs_at_the_start(good, bad, what, sums=True):
    """r at k = 0 differs in bits, and so does row 0 of the inner products (one of them at least: where A x0 is 1e7 times b, as on
    nos7, a single sum of squares can round to the same double for b + A x0 and b - A x0).  sums=False: r alone"""
    (rows, r0), (rows_bad, r0_bad) = good, bad
    assert np.isfinite(rows_bad[0]).all() and np.isfinite(r0_bad).all(), what
    assert np.count_nonzero(r0 != r0_bad) > 0, (what, 'r at k = 0')
    assert not sums or (rows[0] != rows_bad[0]).any(), (what, 'inner products of row 0', rows[0], rows_bad[0])


@pytest.mark.parametrize('method,operator', W.SINGLE_CASES, ids=['-'.join(c) for c in W.SINGLE_CASES])
def test_a_start_up_that_adds_the_product_changes_bits(operators, method, operator):
    """r0 = b + A x0: the subtraction with its operands' sign wrong"""
    A, b, jacobi = operators(operator)
    x0 = W.random_start(A.shape[0])
    good = inner_products(method, A, b, jacobi, x0, 1)
    bad = inner_products(method, A, b, jacobi, x0, 1, A_start=W.FaultyFirstProduct(A, 'plus'))
    assert np.array_equal(bad[1], b + A @ x0) and np.array_equal(good[1], b - A @ x0) and np.count_nonzero(bad[1] != good[1]) > A.shape[0] // 2
    differs_at_the_start(good, bad, (method, operator))
    # ... and from zeros nobody could tell: -(A 0) = -0.0, b - -0.0 = b
    zero = inner_products(method, A, b, jacobi, np.zeros(A.shape[0]), 1)
    zero_bad = inner_products(method, A, b, jacobi, np.zeros(A.shape[0]), 1, A_start=W.FaultyFirstProduct(A, 'plus'))
    assert np.array_equal(zero[0], zero_bad[0]) and np.array_equal(zero[1], zero_bad[1])


@pytest.mark.parametrize('method,operator,nranks,transport', W.RANK_CASES, ids=['-'.join(str(q) for q in c) for c in W.RANK_CASES])
def test_a_halo_of_x0_that_was_not_exchanged_changes_bits(method, operator, nranks, transport):
    """every rank multiplies with its own rows of x0 and zeros in its ghost rows: r differs on the boundary rows of every rank, and
    with it row 0 of the inner products -- but on s3_small, whose off-diagonals are 1e-4 of the diagonal and whose halo is 7 rows
    of 20 000: there the sums need not move by a bit, and only r itself, read on every rank right after begin (run_ranks:
    read_start), shows the fault.  That is why the GPU test reads it."""
    from new_cg_variants_amd import partition
    from new_cg_variants_amd import problems as P
    A = TR.OPERATORS[operator][0](P).tocsr()
    n = A.shape[0]
    b = P.reference_rhs(A, n)[0]
    off = TR.OPERATORS[operator][1](nranks)
    offsets = np.asarray(partition.even_offsets(n, nranks) if off is None else off, dtype=np.int64)
    assert offsets.shape == (nranks + 1,) and offsets[0] == 0 and offsets[-1] == n
    x0, jacobi = W.random_start(n), orc.jacobi(A)
    good = inner_products(method, A, b, jacobi, x0, 1)
    bad = inner_products(method, A, b, jacobi, x0, 1, A_start=W.FaultyFirstProduct(A, 'no_halo', offsets))
    differs_at_the_start(good, bad, (method, operator, nranks), sums=operator != 's3_small')
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        assert np.count_nonzero(good[1][lo:hi] != bad[1][lo:hi]) > 0, ('a rank without a wrong row', int(lo), int(hi))
    zero_bad = inner_products(method, A, b, jacobi, np.zeros(n), 1, A_start=W.FaultyFirstProduct(A, 'no_halo', offsets))
    assert np.array_equal(zero_bad[1], b)                            # from zeros nobody could tell


@pytest.mark.parametrize('variant', B.VARIANTS)
def test_a_system_started_from_its_neighbours_vector_changes_bits(matrices, variant):
    """system s of the batch begun from the start vector of system s + 1 (on its own rows): r, mu, nu and rr of row 0 differ"""
    for s, (name, A, b, x0) in enumerate(W.batch_systems(matrices)):
        good = B.oracle_stopped(A, b, variant, 0.0, 0, jacobi=True, x0=x0)
        bad = B.oracle_stopped(A, b, variant, 0.0, 0, jacobi=True, x0=W.batch_start(s + 1, A.shape[0]))
        assert np.array_equal(good['at0']['x'], x0) and np.array_equal(good['at0']['r'], b - A @ x0)
        assert np.count_nonzero(good['at0']['r'] != bad['at0']['r']) > 0, name
        assert (good['scalars'][0, [0, 3, 4]] != bad['scalars'][0, [0, 3, 4]]).all(), name
