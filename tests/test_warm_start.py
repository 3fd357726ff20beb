"""GPU (MI355X): sessions begun from a NONZERO x0 against the oracle (oracle/ne_oracle.py) begun from the same bits, under the
device's own summation order (tests/device_order.py) -- on every begin path: single sessions on window operators, sliced rows
and CSR-adaptive tiles (prcg_solve_begin: begin_pipe, begin_cg, begin_hs_pr), stored-tilde sessions, the one-workgroup solver,
stopped sessions, batches (batch_begin, k_small_batch_init), 2 and 3 ranks (the halo exchange of x0), and the Python layer.
With x0 = 0 the product A x0 is zero and r0 = b exactly: everything that forms r0 = b - A x0 runs in every other test and is
checked by none (tests/warm_start_common.py: the start kinds 'random', 'restart', 'solved' and the tables of cases;
tests/test_warm_start_model.py: the inputs are valid, and these assertions would notice a faulty start-up).

Every test asserts first, bit for bit, the state right after begin: x == x0 and r == b - A x0 (SciPy's product: a row's sum
left to right from +0.0; LongRowOperator where a CSR tile has long rows) -- a failure there is the start-up's, not iteration
1's.  Then the run: the bodies, trees and bars of the cold-start files, unchanged (tests/test_trajectory_oracle.py,
test_trajectory_irregular.py, test_trajectory_stored_tilde.py, test_trajectory_ranks.py: their whole_trajectory functions;
single_stop_common.py; small_batch_common.py; small_batch_blocks_common.py).  No tolerance of its own: bit for bit, and for
the recorder histories the 1e-13 / 1e-11 of the trajectory tests.  Runs are 60 iterations.

Not here: multi-RHS sessions, whose x0_nonzero cases (tests/multi_rhs_common.py: problem) hold their start-up."""
import numpy as np
import pytest

import small_batch_blocks_common as BB
import small_batch_common as B
import test_gpu_parity as GP
import test_single_stop as SS
import test_trajectory_irregular as TI
import test_trajectory_oracle as TO
import test_trajectory_ranks as TR
import test_trajectory_stored_tilde as TS
import warm_start_common as W
from device_order import device_dot
from single_stop_common import CONVERGED, METHODS as STOP_METHODS, holds_trajectory, run_session, same_reading, stop_of, trajectory
from trajectory_common import holds_start

pytestmark = pytest.mark.gpu

# the module-scoped fixtures of the cold-start files, under names of their own (each builds its operators once and leaves them unchanged)
window_problem, irregular_problem, ranks_problem, stop_problem = TO.problem, TI.problem, TR.problem, SS.problem
irregular_trees, tilde_trees = TI.trees, TS.trees
problem, preconditioner = TS.problem, TS.preconditioner       # (TS.preconditioner asks for `problem`)


@pytest.fixture(scope='module')
def amd():
    import new_cg_variants_amd.callbacks as cbs
    import new_cg_variants_amd.cg_variants as cgv
    from new_cg_variants_amd import _lib, device, problems
    return dict(L=_lib, device=device, problems=problems, cgv=cgv, cbs=cbs)


# ---- c. batches -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def nine(matrices):
    """the nine systems in W.BATCH_ORDER, each with its own random start: built once, never modified"""
    systems = W.batch_systems(matrices)
    for _, _, b, x0 in systems:
        b.setflags(write=False)
        x0.setflags(write=False)
    return systems


def batch_arguments(nine, prec):
    """(blocks, inv_diag) of DeviceBatch.begin and the oracle's prec= per system"""
    precs = [W.batch_prec(A, s, prec) for s, (_, A, _, _) in enumerate(nine)]
    blocks = BB.blocks_of(precs) if prec == 'blocks' else None
    inv_diag = [1 / A.diagonal() for _, A, _, _ in nine] if prec == 'jacobi' else None
    return precs, blocks, inv_diag


@pytest.fixture(scope='module')
def batch_records(amd, nine):
    """(variant, preconditioner) -> the device records of the nine systems, ITERS iterations cut at k = 1"""
    cache = {}

    def get(variant, prec):
        if (variant, prec) not in cache:
            systems, x0s = [(A, b) for _, A, b, _ in nine], [x0 for _, _, _, x0 in nine]
            if prec == 'none':
                cache[(variant, prec)] = B.run_stopping_batch(amd, systems, variant, None, (1, W.ITERS - 1), jacobi=False, x0s=x0s)
            else:
                _, blocks, inv_diag = batch_arguments(nine, prec)
                cache[(variant, prec)] = BB.run_blocks(amd, systems, variant, blocks, (1, W.ITERS - 1), inv_diag=inv_diag, x0s=x0s)
        return cache[(variant, prec)]
    return get


def holds_batch_start(rec, A, b, x0, what):
    holds_start((rec['at0']['x'], rec['at0']['r']), 'xr', x0, b, A, what=f'{what}: ')


def holds_free_run(rec, run, variant, total, what):
    """a device record of small_batch_blocks_common.run_blocks against its trajectory() of `total` iterations, bit for bit with
    NaNs equal (a run that breaks down goes on on both sides: tests/test_small_batch_jacobi.py holds bcsstm22 this way)"""
    idx, ncoef = B.slots(variant), 2 if variant == 'HS' else 3
    assert (rec['k_stop'], rec['status']) == (-1, 0), what
    for k in (0, 1, total):
        for v in run['vec'][k]:
            assert np.array_equal(rec['vec'][k][v], run['vec'][k][v], equal_nan=True), (what, k, v)
    assert rec['scalars'].shape == (total + 1, 8) and rec['coef'].shape == (total, 3) and rec['hist'].shape == (total + 1,)
    bad = ~((rec['scalars'][:, idx] == run['scalars'][:, idx]) | (np.isnan(rec['scalars'][:, idx]) & np.isnan(run['scalars'][:, idx])))
    assert not bad.any(), (what, f'scalars: first mismatch at k={int(np.argmax(bad.any(axis=1)))}')
    assert np.array_equal(rec['coef'][:, :ncoef], run['coef'][:, :ncoef], equal_nan=True), (what, 'coefficients')
    assert np.array_equal(rec['hist'], run['hist'], equal_nan=True), (what, 'history')


@pytest.mark.parametrize('prec', W.BATCH_PRECS)
@pytest.mark.parametrize('variant', B.VARIANTS)
def test_every_system_of_a_batch_from_its_own_start(nine, batch_records, variant, prec):
    """The nine systems, register and LDS systems interleaved so that slot[s] != s for most s -- asserted from the planner hook's
    modes through W.slots_of, a RESTATEMENT of prcg_batch_create's descriptor order (mode 1 first, then mode 0, each in system
    order): the hook returns mode and group, not the slots, so a change of that order in the library would go unnoticed here --,
    every system from its own random x0: x == x0 and r == b - A x0 at k = 0, then each system's own oracle under wg_dot bit
    for bit -- vectors at k = 0, 1 and the end, all scalar and coefficient rows, the history.  Every oracle run is asserted
    clean for all 60 iterations, but bcsstm22 under a preconditioner (diagonal: exact after one step; W.BCSSTM22_BREAKS, asserted
    against this test's own oracle run): held over all 60 iterations with NaNs equal, as the cold-start Jacobi batch tests hold it."""
    rc, mode, _ = B.plan([B.shape_of(A) for _, A, _, _ in nine], jacobi=prec != 'none')
    slot = W.slots_of(mode)
    assert rc == 2 and sum(q != s for s, q in enumerate(slot)) >= 7, slot
    recs = batch_records(variant, prec)
    precs, _, _ = batch_arguments(nine, prec)
    for s, ((name, A, b, x0), rec, M) in enumerate(zip(nine, recs, precs)):
        what = f'{variant} {prec} system {s} ({name}, slot {slot[s]})'
        holds_batch_start(rec, A, b, x0, what)
        if prec == 'none':
            want = B.oracle_stopped(A, b, variant, 0.0, W.ITERS, jacobi=False, x0=x0)
            assert want['status'] == 0 and W.first_bad(want['scalars']) < 0, (what, 'the oracle breaks down', want['k_stop'])
            want.update(k_stop=-1)
            B.holds_oracle(rec, want, variant, W.ITERS, what)
            continue
        run, _ = BB.trajectory(A, b, variant, M, free=W.ITERS, x0=x0)
        kb = W.first_bad(run['scalars'])
        assert kb == (W.BCSSTM22_BREAKS.get((variant, prec), -1) if name == 'bcsstm22' else -1), (what, f'the oracle breaks down at k={kb}')
        assert np.isfinite(run['hist'][:kb if kb > 0 else None]).all() and run['hist'][0] > 0, what       # NaNs cannot carry the test
        holds_free_run(rec, run, variant, W.ITERS, what)


@pytest.mark.parametrize('variant', ['PIPE_PR', 'HS'])
@pytest.mark.parametrize('name', ['nos7', '494_bus'])
def test_one_matrix_three_systems_three_starts(amd, matrices, variant, name):
    """mat_of = [0, 0, 0], the same b, three different x0 (Jacobi): three different trajectories, each its own oracle's -- an x0
    pointer that followed the matrix instead of the system would give three equal ones"""
    A, b = B.system(matrices, name)
    x0s = [W.batch_start(s, A.shape[0]) for s in range(3)]
    recs = B.run_stopping_batch(amd, [(A, b)] * 3, variant, None, (W.ITERS,), mat_of=[0, 0, 0], matrices=[A], x0s=x0s)
    for s, (rec, x0) in enumerate(zip(recs, x0s)):
        holds_batch_start(rec, A, b, x0, f'system {s}')
        want = B.oracle_stopped(A, b, variant, 0.0, W.ITERS, x0=x0)
        assert want['status'] == 0, (s, 'the oracle breaks down', want['k_stop'])
        want.update(k_stop=-1)
        B.holds_oracle(rec, want, variant, W.ITERS, f'{name} system {s}')
    assert len({rec['hist'].tobytes() for rec in recs}) == 3


@pytest.mark.parametrize('variant', B.VARIANTS)
def test_a_solved_system_among_running_ones(amd, nine, variant):
    """rtol = 1e-8, Jacobi: two systems in the middle, one with its matrix in LDS (494_bus) and one in registers (nos7), have
    b' = A x0, so r0 = 0 -- exactly, only if k_small_batch_init's row loop sums a row left to right from +0.0 as SciPy does --:
    converged at 0 with x == x0 and nothing written beyond row 0, while their neighbours, from their random starts, run on and
    equal their stopping oracles (thr from ||b||, not ||r0||)"""
    total = 100
    picked = [nine[i] for i in (0, 1, 6, 3, 4, 5)]               # bcsstk03, 494_bus (LDS, solved), nos7 (registers, solved), model_48_8_3, ...
    solved = (1, 2)                                              # rows of up to 10 and 7 entries: r0 = 0 only if the row loop sums as SciPy does
    systems = [(A, W.solved_rhs(A, x0) if i in solved else b) for i, (_, A, b, x0) in enumerate(picked)]
    x0s = [x0 for _, _, _, x0 in picked]
    thr = B.thresholds([b for _, b in systems], rtol=1e-8)
    assert (thr > 0).all()
    recs = B.run_stopping_batch(amd, systems, variant, thr, (total,), x0s=x0s)
    for s, ((A, b), x0, rec) in enumerate(zip(systems, x0s, recs)):
        holds_batch_start(rec, A, b, x0, f'system {s}')
        want = B.oracle_stopped(A, b, variant, thr[s], total, x0=x0)
        B.holds_oracle(rec, want, variant, total, f'{variant} system {s}')
        if s in solved:
            assert (rec['k_stop'], rec['status']) == (0, CONVERGED) and np.array_equal(rec['at']['x'], x0) and not rec['at']['r'].any()
            assert not rec['scalars'][1:].any() and not rec['hist'].any()
        else:
            assert rec['k_stop'] != 0 and rec['hist'][0] ** 2 > thr[s] and np.isfinite(rec['hist']).all()


def test_the_batch_function_takes_every_systems_start(amd, nine, batch_records):
    """cg_variants.pipe_pr_pcg_batch(As, bs, x0s, ...) with nine distinct nonzero x0s: each trial's history is the DeviceBatch
    session's from the same vectors"""
    cgv, cbs = amd['cgv'], amd['cbs']
    As, bs, x0s = [A for _, A, _, _ in nine], [b for _, _, b, _ in nine], [x0 for _, _, _, x0 in nine]
    keep = [x0.copy() for x0 in x0s]
    out = cgv.pipe_pr_pcg_batch(As, bs, x0s, W.ITERS + 1, preconditioner=[cgv.Jacobi(A) for A in As], callbacks=[cbs.updated_residual_2_norm])
    recs = batch_records('PIPE_PR', 'jacobi')
    assert len(out) == 9
    for s, (trial, rec) in enumerate(zip(out, recs)):
        assert np.array_equal(trial['updated_residual_2_norm'], rec['hist'], equal_nan=True) and np.isfinite(rec['hist'][:5]).all(), s
    assert all(np.array_equal(a, c) for a, c in zip(x0s, keep))
    assert len({trial['updated_residual_2_norm'][:5].tobytes() for trial in out}) == 9


# ---- a. single sessions on one GPU ----------------------------------------------------------------------------------------------
def pr_knobs(method, operator):
    """the packed / unpacked form of the unpreconditioned predict-and-recompute launch, as test_trajectory_oracle.py's table sets
    it: packed on the one-tile operator, unpacked where the packed launch and the one a recorder forces are different trees"""
    if method not in ('pr_cg', 'm_cg') or operator not in W.WINDOW_OPERATORS:
        return {}
    return TO.PACK if operator == 'bcsstk03' else TO.UNPACK


@pytest.mark.parametrize('kind', ['random', 'restart'])
@pytest.mark.parametrize('method,operator', W.SINGLE_CASES, ids=['-'.join(c) for c in W.SINGLE_CASES])
def test_whole_trajectory_of_a_single_session_from_a_start_vector(amd, window_problem, irregular_problem, irregular_trees, method, operator, kind):
    """the bodies of test_whole_trajectory_of_the_default_schedule (window operators) and
    test_whole_trajectory_on_sliced_rows_and_csr_tiles with x0: both modes -- (a) all four recorders, whose k = 0 entries are the
    norms of x_true - x0 and of the true residual of x0; (b) chunks of 1, 2, 37 iterations and the rest -- 60 iterations"""
    if operator in W.WINDOW_OPERATORS:
        TO.whole_trajectory(amd, window_problem, method, operator, W.ITERS, pr_knobs(method, operator), x0=W.STARTS[kind])
    else:
        TI.whole_trajectory(amd, irregular_problem, irregular_trees, method, operator, {}, x0=W.STARTS[kind], max_iter=W.ITERS)


@pytest.mark.parametrize('kind', ['random', 'restart'])
@pytest.mark.parametrize('method,operator,prec', W.STORED_TILDE_CASES, ids=['-'.join(c) for c in W.STORED_TILDE_CASES])
def test_whole_trajectory_of_a_stored_tilde_session_from_a_start_vector(amd, problem, preconditioner, tilde_trees, method, operator, prec, kind):
    """the body of test_whole_trajectory_of_the_stored_tilde_schedule with x0: BlockJacobi(A, 3) on sliced rows; the stored r~,
    s~, u~, w~ right after begin are the oracle's"""
    TS.whole_trajectory(amd, problem, preconditioner, tilde_trees, method, operator, prec, W.ITERS, x0=W.STARTS[kind])


@pytest.mark.parametrize('variant,matrix', W.SMALL_SOLVER_CASES, ids=['-'.join(c) for c in W.SMALL_SOLVER_CASES])
def test_one_workgroup_solver_from_a_start_vector(amd, matrices, variant, matrix):
    """the body of test_gpu_parity.py::test_one_workgroup_solver_for_small_systems from the random start (default PRCG_SMALL, the
    recurrence residual only), held exactly as the cold start is: x == x0 and r == b - A x0 after begin on both handles; 30 forced
    steps from the multi-launch schedule's state -- vectors bit for bit (Hestenes-Stiefel's p and s to 1e-12), inner products to
    1e-12; 3000 free-running iterations, the same history in one call and in pieces; against the multi-launch run the history
    holds 1e-12 on the rows below W.WARM_PREFIX_FLOOR (6 on bcsstk03, 13 on nos7: one iteration below where the reference's own
    re-ordered sums part from this start, measured by tests/test_warm_start_model.py; the cold start's floors are 7 / 15).  The
    body prints the first k at which the two histories do part."""
    A = matrices[matrix][0]
    GP.one_workgroup_solver(amd, matrices, matrix, variant, x0=W.random_start(A.shape[0]), prefix_floor=W.WARM_PREFIX_FLOOR)


# ---- b. stopped single sessions -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['random', 'restart'])
@pytest.mark.parametrize('method', W.STOP_METHODS)
@pytest.mark.parametrize('operator', W.STOP_OPERATORS)
def test_a_session_from_a_start_vector_stops_where_the_oracle_does(amd, stop_problem, operator, method, kind):
    """A window, a sliced-row and a CSR-tile operator of test_single_stop.py's table.  thr = (rtol ||b||_2)^2, the expression of
    cg_variants: relative to b, not to r0 (W.STOP_RUN: rtol and max_iter per case).  The oracle runs from x0 under the tree of the
    layout the session reports, the rule is applied to its rows in Python; asserted: it fires, converged, at an interior k.
    Sessions: without a threshold (the whole run); rr_stop = thr in one call, then three more iterations (a no-op); calls of
    k_stop and the rest.  Each holds the oracle's state bit for bit: stop word, vectors, scalars, coefficients, history."""
    L = amd['L']
    _, _, jac = STOP_METHODS[method]
    A, b, inv_diag = stop_problem(operator)
    d = inv_diag if jac else None
    max_iter, rtol = W.STOP_RUN[(operator, method, kind)]
    thr = float(B.thresholds([b], rtol=rtol)[0])
    op = SS.open_operator(amd, A, operator)
    try:
        x0 = W.STARTS[kind](op, A, b)
        free = run_session(L, op, method, b, d, max_iter, None, (max_iter - 1,), x0=x0)
        holds_start(free['start'], 'xr', x0, b, A, what='no threshold: ')
        dot = SS.check_family(A, operator, jac, free)
        traj = trajectory(A, b, method, dot, device_dot, max_iter - 1, keep=(), x0=x0)
        k_stop, status = stop_of(traj, thr)
        print(f'{operator} {method} from {kind}: rtol = {rtol}, thr = {thr!r}, rr at k = 0 {traj["scalars"][0, 4]!r}; the oracle stops at k = {k_stop} '
              f'with status {status}')
        assert status == CONVERGED and 0 < k_stop < max_iter - 1, (k_stop, status)
        assert traj['scalars'][0, 4] > thr and np.isfinite(traj['scalars'][:k_stop + 1]).all()
        assert stop_of(traj, 0.0) == (-1, 0), 'the run breaks down before its end'
        traj = trajectory(A, b, method, dot, device_dot, max_iter - 1, keep=(k_stop, max_iter - 1), x0=x0)
        holds_trajectory(free, traj, max_iter - 1, 0, max_iter, 'no threshold')
        one = run_session(L, op, method, b, d, max_iter, thr, (max_iter - 1,), then=3, x0=x0)
        cut = run_session(L, op, method, b, d, max_iter, thr, (k_stop, max_iter - 1 - k_stop), x0=x0)
    finally:
        op.close()
    for what, rec in (('one call', one), ('a call ends at k_stop', cut)):
        holds_start(rec['start'], 'xr', x0, b, A, what=what + ': ')
        assert SS.same_launch(rec, free), (what, rec['schedule'])
        holds_trajectory(rec, traj, k_stop, status, max_iter, what)
    assert same_reading(one, one['again']), 'prcg_iterate on a stopped session is a no-op'


@pytest.mark.parametrize('method', W.STOP_METHODS)
@pytest.mark.parametrize('operator', W.STOP_OPERATORS)
def test_a_solved_start_is_converged_before_the_first_iteration(amd, stop_problem, operator, method):
    """b' = A x0 (rows summed left to right from +0.0: no operator here has long rows), so r0 = 0 exactly.  thr = 0: rr = 0 <= 0 on
    row 0 -- converged at 0, x carries the bits of x0, no row beyond 0 is written, later prcg_iterate calls change nothing
    (begin_pipe: "b = A x0 stops the session before its first iteration").  Without a threshold: 0 / 0 at the first step, the
    history fills with NaN and no call raises, as test_gpu_parity.py::test_breakdown_propagates_nan_not_exception pins it for
    b = 0, x0 = 0."""
    L = amd['L']
    _, _, jac = STOP_METHODS[method]
    A, _, inv_diag = stop_problem(operator)
    d = inv_diag if jac else None
    x0 = W.random_start(A.shape[0])
    b = W.solved_rhs(A, x0)
    max_iter = 9
    op = SS.open_operator(amd, A, operator)
    try:
        rec = run_session(L, op, method, b, d, max_iter, 0.0, (3, 5), then=2, x0=x0)
        free = run_session(L, op, method, b, d, max_iter, None, (max_iter - 1,), x0=x0)
    finally:
        op.close()
    for r in (rec, free):
        holds_start(r['start'], 'xr', x0, b, A)
        assert not r['start'][1].any()
    assert rec['stop'] == (0, CONVERGED) and rec['k'] == 0
    assert np.array_equal(rec['at']['x'], x0)
    assert all(np.array_equal(v, np.zeros(A.shape[0])) for name, v in rec['at'].items() if name != 'x'), [name for name, v in rec['at'].items() if v.any()]
    assert np.array_equal(rec['scalars'], np.zeros((max_iter, 8))) and np.array_equal(rec['coef'], np.zeros((max_iter - 1, 3)))
    assert np.array_equal(rec['hist'], np.zeros(max_iter))
    assert same_reading(rec, rec['again'])
    assert free['stop'] == (-1, 0) and free['k'] == max_iter - 1
    assert free['hist'][0] == 0.0 and np.all(np.isnan(free['hist'][1:]))


# ---- e. the Python layer --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,variant,jac', [('pipe_pr_cg', 'PIPE_PR', False), ('hs_pcg', 'HS', True)])
@pytest.mark.parametrize('operator', ['nos7', 'fem12'])
def test_cg_variants_take_x0_contiguous_or_not(amd, stop_problem, operator, name, variant, jac):
    """cg_variants.pipe_pr_cg / hs_pcg (Jacobi) with x0 as a contiguous array and as a non-contiguous view of the same values: the
    history, x at k = 0 and x at the end are those of a DeviceCSR.begin session from that vector (default knobs, as the functions
    open their operator), and the caller's array is unchanged (the reference copies it: hs_cg.py:22)"""
    cgv, cbs, L = amd['cgv'], amd['cbs'], amd['L']
    A, b, inv_diag = stop_problem(operator)
    n = A.shape[0]
    x0 = W.random_start(n)
    wide = np.zeros(2 * n)
    wide[::2] = x0
    view = wide[::2]
    assert not view.flags.c_contiguous and np.array_equal(view, x0)
    keep, keep_wide = x0.copy(), wide.copy()
    op = amd['device'].DeviceCSR(A)
    try:
        op.begin(getattr(L, variant), b, x0, W.ITERS, inv_diag=inv_diag if jac else None, hist_mask=1)
        holds_start((op.get_vector('x'), op.get_vector('r')), 'xr', x0, b, A)
        op.iterate(W.ITERS - 1)
        op.sync()
        hist, x_end = op.history()['updated_residual_2_norm'], op.get_vector('x')
    finally:
        op.close()
    assert np.isfinite(hist).all() and (hist > 0).all()
    kw = {'preconditioner': cgv.Jacobi(A)} if jac else {}
    cgv.clear_operator_cache()
    try:
        for what, arg in (('contiguous', x0), ('view', view)):
            out = getattr(cgv, name)(A, b, arg, W.ITERS, callbacks=[cbs.updated_residual_2_norm], **kw)
            assert np.array_equal(out['updated_residual_2_norm'], hist), what
            seen = {}

            def foreign(**env):
                seen[env['k']] = env['x_k'].copy()
            out = getattr(cgv, name)(A, b, arg, W.ITERS, callbacks=[cbs.updated_residual_2_norm, foreign], **kw)
            assert sorted(seen) == list(range(W.ITERS)), what
            assert np.array_equal(seen[0], x0) and np.array_equal(seen[W.ITERS - 1], x_end), what
            assert np.array_equal(out['updated_residual_2_norm'], hist), what
            assert np.array_equal(x0, keep) and np.array_equal(wide, keep_wide), (what, 'the caller\'s x0 was written')
    finally:
        cgv.clear_operator_cache()


# ---- d. several ranks -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method,operator,nranks,transport', W.RANK_CASES, ids=['-'.join(str(q) for q in c) for c in W.RANK_CASES])
def test_whole_trajectory_of_a_multi_rank_session_from_a_start_vector(amd, ranks_problem, method, operator, nranks, transport):
    """the body of test_whole_trajectory_of_a_multi_rank_session (rank threads on one GPU, one case at a time) from a random GLOBAL
    x0: every rank's ghost rows of x0 are nonzero, and every rank's rows of r read right after begin (run_ranks: read_start) are
    the global b - A x0 -- the halo exchange of x0 inside the start-up product, by each transport's own path.  No breakdown
    table: the case asserts that its own oracle run has finite, positive mu and nu at all 60 iterations."""
    A = ranks_problem(operator)[0]
    TR.whole_trajectory(amd, ranks_problem, method, operator, nranks, transport, W.ITERS, x0=W.random_start(A.shape[0]))
