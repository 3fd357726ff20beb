"""A single HESTENES-STIEFEL session stops at a residual threshold, decided on the device (prcg.h: prcg_set_stop_hs, prcg_get_stop;
device.DeviceCSR.begin(L.HS, rr_stop=...), .stop(); cg_variants.hs_cg_stop / hs_pcg_stop).

The yardstick is the oracle's free-running hs_cg / hs_pcg trajectory under the device's own summation order (hs_stop_common:
which launch sums what), with the stopping rule applied to its rows in Python (single_stop_common.stop_of: small_batch_common.rule,
the batch's).  Everything is compared for equal bits.  Thresholds come from the oracle: thr = its rr at iteration max_iter // 2; the
stop is the first k the rule fires at.  The cases are the smallest that reach each launch family (hs_stop_common.CASES; found on
the CPU with the oracle under np.dot, tests/test_hs_stop_model.py, and asserted here again under the device's tree):

  s3_small, s1_small, laplace_3d(21,17,13) with PRCG_SMALL=0   window tiles (s3_small: value dictionary): k_hs_update_xr_stop, launch_win_hs
  fem_like_3d(12)                                               sliced rows, window codes: + k_hs_update_p_stop, k_sell_win
  fem_irregular_3d(10) with PRCG_SELL_WINDOW=0                  sliced rows, gathers: k_sell_tiles
  bcsstk14 with PRCG_SELL=0                                     CSR-adaptive tiles: k_spmv_tiles
  bcsstk03, nos4, laplace_2d(27,27), laplace_2d(2100,1),        the one-workgroup solver (n = 112, 100, 729, 2100: three rows per thread),
  default knobs                                                 hs_cg only: with Jacobi a single session takes the window tiles
  s1_small, default knobs                                       n = 3072 does NOT fit the one-workgroup solver (280 KB of matrix and vectors
                                                                against its 156 KB): window tiles again, as the schedule says
nos7 without a preconditioner is not among them: its residual grows for hundreds of iterations, so any thr taken from its
trajectory stops at k = 0."""
import ctypes as C
import re

import numpy as np
import pytest

from hs_stop_common import (BREAKDOWN, BREAKDOWNS, CASES, CONVERGED, METHODS, OPERATORS, case_id, holds_trajectory, make_problem,
                            oracle_sums, run_session, same_launch, same_reading, stop_of, trajectory)


@pytest.fixture(scope='module')
def amd():
    from new_cg_variants_amd import _lib, device, problems
    return dict(L=_lib, device=device, problems=problems)


@pytest.fixture(scope='module')
def problem(amd, matrices):
    return make_problem(amd['problems'], matrices)


def open_operator(amd, A, operator):
    return amd['device'].DeviceCSR(A, knobs=dict(OPERATORS[operator][0]))


@pytest.mark.gpu
@pytest.mark.parametrize('operator,method,max_iter', CASES, ids=[case_id(c) for c in CASES])
def test_a_session_stops_where_the_oracle_does(amd, problem, operator, method, max_iter):
    """Five sessions on one handle.  (0) without a threshold, one prcg_iterate call: its layouts give the oracle's trees, the
    oracle gives thr = rr at max_iter // 2 and the stop.  (1) rr_stop = thr, one prcg_iterate(max_iter - 1) call: the stop is decided
    by the prologue of launch A of iteration k_stop + 1 (one-workgroup solver: inside its loop).  (2a) calls of k_stop and the rest:
    the reduction that ends the first call decides; (2b) calls of k_stop + 1 and the rest: the prologue of launch A of that call's
    last iteration.  No synchronisation between the calls: the later launches find the session stopped.  (3) a further
    prcg_iterate(3) after (1) changes nothing.  All three hold the oracle's state at k_stop bit for bit: stop word, x r p s (r~),
    scalar rows 0..k_stop, coefficient rows 1..k_stop, the history; everything beyond reads zero; prcg_iteration is k_stop.
    (4) thr = 0: never stops, and every vector, scalar, coefficient and history entry equals session (0)."""
    L = amd['L']
    jac = METHODS[method]
    A, b, inv_diag = problem(operator)
    d = inv_diag if jac else None
    op = open_operator(amd, A, operator)
    try:
        free = run_session(L, op, method, b, d, max_iter, None, (max_iter - 1,))
        sums, sums0 = oracle_sums(A, operator, jac, free)
        traj = trajectory(A, b, method, sums, sums0, max_iter - 1, keep=())
        thr = float(traj['scalars'][max_iter // 2, 4])
        k_stop, status = stop_of(traj, thr)
        print(f'{case_id((operator, method, max_iter))}: thr = {thr!r}, the oracle stops at k = {k_stop} with status {status}; '
              f'{free["layout"]["grid"]} workgroups x {free["layout"]["waves_per_block"]} waves')
        assert np.isfinite(thr) and thr > 0 and 0 < k_stop < max_iter - 1 and status in (CONVERGED, BREAKDOWN), (thr, k_stop, status)
        assert np.isfinite(traj['scalars'][:k_stop + 1]).all() and np.isfinite(traj['coef'][:k_stop]).all()
        assert stop_of(traj, 0.0) == (-1, 0), 'the run breaks down: a wrong case for the thr = 0 comparison'
        traj = trajectory(A, b, method, sums, sums0, max_iter - 1, keep=(k_stop, max_iter - 1))
        assert all(np.isfinite(v).all() for v in traj['at'][k_stop].values())
        holds_trajectory(free, traj, max_iter - 1, 0, max_iter, 'no threshold')
        rest = max_iter - 1 - k_stop
        one = run_session(L, op, method, b, d, max_iter, thr, (max_iter - 1,), then=3)
        at_end = run_session(L, op, method, b, d, max_iter, thr, (k_stop, rest))
        past = run_session(L, op, method, b, d, max_iter, thr, (k_stop + 1, rest - 1))
        never = run_session(L, op, method, b, d, max_iter, 0.0, (max_iter - 1,))
    finally:
        op.close()
    for what, rec in (('one call', one), ('a call ends at k_stop', at_end), ('a call ends at k_stop + 1', past)):
        assert rec['schedule'] == free['schedule'] and same_launch(rec, free), (what, rec['schedule'])
        holds_trajectory(rec, traj, k_stop, status, max_iter, what)
    assert same_reading(one, one['again']), 'prcg_iterate on a stopped session is a no-op'
    assert never['schedule'] == free['schedule'] and same_launch(never, free)
    assert never['stop'] == (-1, 0) and never['k'] == max_iter - 1
    assert same_reading(never, free), 'thr = 0 on a run that does not stop: the bits of the session without a threshold'


@pytest.mark.gpu
def test_a_jacobi_session_of_a_small_system_takes_the_window_tiles(amd, problem):
    """bcsstk03 (n = 112) with default knobs: hs_cg runs on the one-workgroup solver, hs_pcg does not select it (a follow-up) -- with
    a threshold the schedule says so, and the session stops where its own free run first satisfies the rule"""
    L = amd['L']
    A, b, inv_diag = problem('bcsstk03_wg')
    max_iter = 40
    op = open_operator(amd, A, 'bcsstk03_wg')
    try:
        free = run_session(L, op, 'hs_pcg', b, inv_diag, max_iter, None, (max_iter - 1,))
        thr = float(free['scalars'][max_iter // 2, 4])
        k_stop, status = stop_of(dict(scalars=free['scalars'][:, :5]), thr)
        rec = run_session(L, op, 'hs_pcg', b, inv_diag, max_iter, thr, (max_iter - 1,))
    finally:
        op.close()
    for r in (free, rec):
        assert r['schedule']['fused'] and r['schedule']['window'] and not r['schedule']['small'], r['schedule']
    assert 0 < k_stop <= max_iter // 2 and status == CONVERGED
    assert rec['stop'] == (k_stop, status) and rec['k'] == k_stop
    assert np.array_equal(rec['scalars'][:k_stop + 1], free['scalars'][:k_stop + 1]) and not rec['scalars'][k_stop + 1:].any()


@pytest.mark.gpu
@pytest.mark.parametrize('operator,method', [('s3_small', 'hs_cg'), ('fem12', 'hs_pcg'), ('bcsstk14', 'hs_pcg'), ('bcsstk03_wg', 'hs_cg')])
def test_a_zero_right_hand_side_stops_before_the_first_iteration(amd, problem, operator, method):
    """b = 0, x0 = 0, thr = 0: rr = 0 <= 0 on row 0 -- stopped at 0, converged, whatever mu is; no row beyond 0 is written"""
    L = amd['L']
    A, b, inv_diag = problem(operator, 'zero')
    max_iter = 9
    op = open_operator(amd, A, operator)
    try:
        rec = run_session(L, op, method, b, inv_diag if METHODS[method] else None, max_iter, 0.0, (3, 5), then=2)
    finally:
        op.close()
    assert rec['stop'] == (0, CONVERGED) and rec['k'] == 0
    assert all(np.array_equal(v, np.zeros(A.shape[0])) for v in rec['at'].values())
    assert np.array_equal(rec['scalars'], np.zeros((max_iter, 8))) and np.array_equal(rec['coef'], np.zeros((max_iter - 1, 3)))
    assert np.array_equal(rec['hist'], np.zeros(max_iter))
    assert same_reading(rec, rec['again'])


@pytest.mark.gpu
@pytest.mark.parametrize('operator,method,max_iter,k_break', BREAKDOWNS, ids=[case_id(c) for c in BREAKDOWNS])
def test_a_breakdown_stops_the_session(amd, problem, operator, method, max_iter, k_break):
    """A symmetric INDEFINITE operator (a shifted 5-point Laplacian) and a threshold far below what the run reaches: mu = p.s turns
    negative at an interior k and the rule stops the session there with status 2 -- on the window tiles (laplace_2d(64,48) - 0.02 I,
    with and without Jacobi, k = 19) and on the one-workgroup solver (laplace_2d(27,27) - 0.05 I, k = 14).  The oracle's status is
    asserted first; x at the stop is finite."""
    L = amd['L']
    jac = METHODS[method]
    A, b, inv_diag = problem(operator)
    d = inv_diag if jac else None
    thr = 1e-300
    op = open_operator(amd, A, operator)
    try:
        free = run_session(L, op, method, b, d, max_iter, None, (max_iter - 1,))       # (nobody stops it)
        sums, sums0 = oracle_sums(A, operator, jac, free)
        traj = trajectory(A, b, method, sums, sums0, max_iter - 1)
        k_stop, status = stop_of(traj, thr)
        print(f'{operator} {method}: the oracle breaks down at k = {k_stop}: mu, nu, rr = {traj["scalars"][k_stop, [0, 3, 4]]}')
        assert (k_stop, status) == (k_break, BREAKDOWN) and traj['scalars'][k_stop, 0] < 0, (k_stop, status)
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
    served, clears = 'which serves PRCG_HS on one GPU', 'prcg_set_stop_hs(h, NULL) clears the threshold'

    def error():
        return lib.prcg_last_error(h).decode()

    def begin(variant, d=None):
        return lib.prcg_solve_begin(h, variant, L.ptr(b), L.ptr(x0), 12, None, L.ptr(d), 1)

    def refused(rc, *texts):
        assert rc == L.EINVAL, rc
        for t in (served, clears) + texts:
            assert t in error(), (t, error())
    try:
        good = np.array([1e-30])
        assert lib.prcg_set_stop_hs(h, L.ptr(good)) == L.OK
        for bad, text in ((np.nan, 'nan'), (np.inf, 'inf'), (-np.inf, '-inf'), (-1e-300, '-1e-300')):
            assert lib.prcg_set_stop_hs(h, L.ptr(np.array([bad]))) == L.EINVAL
            assert re.search(rf'prcg_set_stop_hs: rr_stop = {re.escape(text)}: the threshold must be finite and >= 0', error()), error()
        for variant in (L.PIPE_PR, L.PIPE_PR_M, L.PIPE_P, L.PIPE_P_M, L.PR, L.M, L.CG_CG, L.GV):      # (the value set before stayed)
            refused(begin(variant), f'variant {variant} is not Hestenes-Stiefel')
        assert lib.prcg_get_stop(h, L.ptr(k_stop), L.ptr(status)) == L.EINVAL          # (a refused begin opens nothing)
        op.build_block_jacobi(2)
        refused(begin(L.HS), 'host-callback or block-Jacobi preconditioner is in force')
        assert begin(L.HS, inv_diag) == L.OK               # (inv_diag overrides the blocks: the diagonal scaling is served)
        cols = (C.c_void_p * 2)(L.ptr(b), L.ptr(b))
        zeros = (C.c_void_p * 2)(L.ptr(x0), L.ptr(x0))
        assert lib.prcg_solve_begin_multi_block_jacobi(h, L.HS, 2, cols, zeros, 12, 1) == L.EINVAL
        assert 'prcg_solve_begin_multi_block_jacobi' in error() and 'SINGLE PRCG_HS sessions only' in error() and clears in error(), error()
        op.set_block_jacobi(0, None)
        assert lib.prcg_solve_begin_multi(h, L.HS, 2, cols, zeros, 12, None, 1) == L.EINVAL
        assert 'prcg_solve_begin_multi:' in error() and 'SINGLE PRCG_HS sessions only' in error() and clears in error(), error()
        assert lib.prcg_solve_begin_multi_pipe(h, L.PIPE_PR, 2, cols, zeros, 12, None, 1) == L.EINVAL
        assert 'prcg_solve_begin_multi_pipe:' in error() and 'SINGLE PRCG_HS sessions only' in error(), error()
        fn = L.PREC_FN(lambda ctx, count, v, out: 1)
        assert lib.prcg_set_preconditioner(h, C.cast(fn, C.c_void_p), None) == L.OK
        refused(begin(L.HS), 'host-callback or block-Jacobi preconditioner is in force')
        assert lib.prcg_set_preconditioner(h, None, None) == L.OK
        hook = L.REPLACE_FN(lambda ctx, k: 0)
        assert lib.prcg_set_replace_hook(h, C.cast(hook, C.c_void_p), None) == L.OK
        refused(begin(L.HS), 'a replace hook is set')
        assert lib.prcg_set_replace_hook(h, None, None) == L.OK
        # independent of the other setters: with prcg_set_stop set as well, ITS refusal of PRCG_HS stands
        assert lib.prcg_set_stop(h, L.ptr(good)) == L.OK
        assert begin(L.HS) == L.EINVAL and 'variant 0 is not pipelined' in error(), error()
        assert lib.prcg_set_stop(h, None) == L.OK
        # a session begun with a threshold: running -> {-1, 0}; its state is not set from outside
        assert begin(L.HS) == L.OK
        assert lib.prcg_get_stop(h, L.ptr(k_stop), L.ptr(status)) == L.OK and (k_stop[0], status[0]) == (-1, 0)
        row = np.zeros(8)
        for call, who in ((lambda: lib.prcg_set_vector(h, L.VEC['x'], L.ptr(x0)), 'prcg_set_vector'),
                          (lambda: lib.prcg_set_scalars(h, 0, L.ptr(row)), 'prcg_set_scalars'), (lambda: lib.prcg_set_iteration(h, 0), 'prcg_set_iteration')):
            assert call() == L.EINVAL and f'{who}: the open session was begun with a stop threshold' in error(), (who, error())
        # cleared: everything is served again, a session has no stop, the setters work
        assert lib.prcg_set_stop_hs(h, None) == L.OK
        for variant in (L.HS, L.PIPE_PR, L.PR, L.CG_CG):
            assert begin(variant) == L.OK, error()
        assert lib.prcg_get_stop(h, L.ptr(k_stop), L.ptr(status)) == L.OK and (k_stop[0], status[0]) == (-1, 0)
        assert lib.prcg_set_vector(h, L.VEC['x'], L.ptr(x0)) == L.OK
        assert lib.prcg_solve_begin_multi(h, L.HS, 2, cols, zeros, 12, None, 1) == L.OK, error()
        # the Python route clears the threshold behind its begin: a multi-RHS session right after it is served
        op.begin(L.HS, b, x0, 12, rr_stop=1e-30)
        assert op.stop() == (-1, 0)
        op.begin_multi(L.HS, np.stack([b, b]), np.zeros((2, n)), 12)
        with pytest.raises(L.PrcgError, match='variant 0 is not pipelined'):       # with a callback the route stays prcg_set_stop's
            op.begin(L.HS, b, x0, 12, preconditioner=lambda v: v, rr_stop=1.0)
    finally:
        op.close()
    # PRCG_FUSED=0 selects the schedule with reduction launches, which cannot stop
    op = amd['device'].DeviceCSR(A, knobs={'PRCG_FUSED': '0'})
    try:
        with pytest.raises(L.PrcgError, match='PRCG_FUSED=0 selects the schedule with reduction launches, which cannot stop'):
            op.begin(L.HS, b, x0, 12, rr_stop=1.0)
        op.begin(L.HS, b, x0, 12)
        assert op.stop() == (-1, 0)
    finally:
        op.close()


@pytest.mark.gpu
def test_cg_variants_stop_at_rtol(amd, problem):
    """hs_pcg_stop(..., preconditioner=Jacobi(A), rtol=1e-8) on fem_like_3d(12): 'iterations', 'status' and the history are those of a
    session begun with rr_stop = (rtol ||b||)^2 in one call, which are the oracle's; a foreign callback is called k_stop + 1 times
    -- for k = 0 .. k_stop, on the states of the run -- and never after the stop"""
    import new_cg_variants_amd.callbacks as cbs
    import new_cg_variants_amd.cg_variants as cgv
    L = amd['L']
    A, b, inv_diag = problem('fem12')
    n, max_iter, rtol = A.shape[0], 120, 1e-8
    thr = float(np.maximum(rtol * np.linalg.norm(b), 0.0) ** 2)
    op = open_operator(amd, A, 'fem12')
    try:
        rec = run_session(L, op, 'hs_pcg', b, inv_diag, max_iter, thr, (max_iter - 1,))
        sums, sums0 = oracle_sums(A, 'fem12', True, rec)
    finally:
        op.close()
    traj = trajectory(A, b, 'hs_pcg', sums, sums0, max_iter - 1, keep=())
    k_stop, status = stop_of(traj, thr)
    print(f'fem12 hs_pcg rtol = {rtol}: thr = {thr!r}, the oracle stops at k = {k_stop} with status {status}')
    assert 0 < k_stop < max_iter - 1 and status in (CONVERGED, BREAKDOWN)
    assert rec['stop'] == (k_stop, status) and rec['k'] == k_stop
    assert np.array_equal(rec['hist'][:k_stop + 1], np.sqrt(traj['scalars'][:k_stop + 1, 4])) and not rec['hist'][k_stop + 1:].any()
    cgv.clear_operator_cache()
    try:
        out = cgv.hs_pcg_stop(A, b, np.zeros(n), max_iter, preconditioner=cgv.Jacobi(A), rtol=rtol, callbacks=[cbs.updated_residual_2_norm])
        assert out['iterations'] == k_stop and out['status'] == ('converged' if status == CONVERGED else 'breakdown')
        assert np.array_equal(out['updated_residual_2_norm'], rec['hist'])
        seen = []

        def foreign(**env):
            seen.append((env['k'], float(env['nu_k']), env['x_k'].copy()))
        out2 = cgv.hs_pcg_stop(A, b, np.zeros(n), max_iter, preconditioner=cgv.Jacobi(A), rtol=rtol, callbacks=[cbs.updated_residual_2_norm, foreign])
        assert [k for k, _, _ in seen] == list(range(k_stop + 1)), [k for k, _, _ in seen]
        assert [nu for _, nu, _ in seen] == traj['scalars'][:k_stop + 1, 3].tolist()
        assert out2['iterations'] == k_stop and out2['status'] == out['status']
        assert np.array_equal(out2['updated_residual_2_norm'], rec['hist'])
        assert np.array_equal(seen[-1][2], rec['at']['x'])
        # without the keywords: no stop, no new keys -- hs_pcg / hs_cg, bit for bit
        out3 = cgv.hs_pcg_stop(A, b, np.zeros(n), 12, preconditioner=cgv.Jacobi(A), callbacks=[cbs.updated_residual_2_norm])
        ref3 = cgv.hs_pcg(A, b, np.zeros(n), 12, preconditioner=cgv.Jacobi(A), callbacks=[cbs.updated_residual_2_norm])
        assert 'iterations' not in out3 and 'status' not in out3 and np.array_equal(out3['updated_residual_2_norm'], ref3['updated_residual_2_norm'])
        assert (out3['updated_residual_2_norm'] > 0).all()
        out3 = cgv.hs_cg_stop(A, b, np.zeros(n), 12, callbacks=[cbs.updated_residual_2_norm])
        ref3 = cgv.hs_cg(A, b, np.zeros(n), 12, rtol=1e-8, callbacks=[cbs.updated_residual_2_norm])          # (hs_cg passes rtol= by)
        assert 'iterations' not in out3 and 'iterations' not in ref3 and np.array_equal(out3['updated_residual_2_norm'], ref3['updated_residual_2_norm'])
        # atol alone, far above the initial residual: stopped at 0
        out4 = cgv.hs_cg_stop(A, b, np.zeros(n), 12, atol=1e3 * np.linalg.norm(b), callbacks=[cbs.updated_residual_2_norm])
        assert out4['iterations'] == 0 and out4['status'] == 'converged' and not out4['updated_residual_2_norm'][1:].any()
        # a run that ends before the threshold is reached
        out5 = cgv.hs_cg_stop(A, b, np.zeros(n), 6, rtol=1e-30, callbacks=[cbs.updated_residual_2_norm])
        assert out5['iterations'] == 5 and out5['status'] == 'max_iter' and (out5['updated_residual_2_norm'] > 0).all()
    finally:
        cgv.clear_operator_cache()
