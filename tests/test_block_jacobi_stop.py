"""A pipelined single session WITH POINT-BLOCK JACOBI stops at a residual threshold, decided on the device (prcg.h:
prcg_set_stop_block_jacobi; device.DeviceCSR.begin(block_jacobi= | block_jacobi_var=, rr_stop=); cg_variants.pipe_*_bpcg(rtol=, atol=)).

Such a session runs the stored-tilde schedule (tests/test_trajectory_stored_tilde.py): per iteration an update launch, the
reduction of its partial rows, the product, one launch that applies the blocks to w and u.  With a threshold each of the four
is a stop form on the session's word: update k is skipped if the session stopped at k - 1 or earlier; the reduction sums row k
and applies the rule; product k and pair launch k belong to the state of k and are skipped only if the session stopped before k.

The yardstick is the oracle (oracle/ne_oracle.py: pipe_start / pipe_advance with prec= the block object -- for blocks built on
the device the blocks read back) with every inner product and r.r summed by device_order.device_dot, the pipelined update
tree, and the rule applied to its rows in Python (single_stop_common: rule, stop_of).  Everything is compared for equal bits
(single_stop_common.holds_trajectory): the stop word, prcg_iteration, the ten vectors x r p s w u r~ s~ u~ w~ of the stop state,
scalar rows 0..k_stop and coefficient rows 1..k_stop, zeros beyond, the history.  Every handle: PRCG_SMALL=0.

The cases and their thresholds are block_jacobi_stop_common.CASES; where the oracle stops is computed here, never written
down: each case asserts 0 < k_stop < max_iter - 6, so that "zero beyond the stop" and the further iterate(5) mean something.
On the CPU the oracle of the table stopped at k = 68, 51, 88, 88, 89, 94 (breakdown), 90 (breakdown), 99 (breakdown), 152, 123."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from block_jacobi_stop_common import (BLOCKS, BREAKDOWN, CASES, CHUNKS, CONVERGED, FLAVOUR, SYSTEMS, VECTORS, begin_keyword, block_object,
                                      case_id, cyclic_partition, run_session, system, threshold, trajectory, with_blocks_read_back)
from device_order import device_dot
from single_stop_common import holds_trajectory, same_reading, stop_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BPCG = ['pipe_pr_bpcg', 'pipe_pr_m_bpcg', 'pipe_p_bpcg', 'pipe_p_m_bpcg']


@pytest.fixture(scope='module')
def amd():
    import new_cg_variants_amd.cg_variants as cgv
    from new_cg_variants_amd import _lib, device
    return dict(L=_lib, device=device, cgv=cgv)


def open_operator(amd, A, name):
    return amd['device'].DeviceCSR(A, knobs=dict(SYSTEMS[name][1], PRCG_SMALL='0'))


def oracle_of(matrices, case, M=None):
    """(A, b, thr, M, trajectory up to its stop, k_stop, status) of a case; M: the object to apply (default: the host object)"""
    name, blocks, variant, rtol, max_iter, _ = case
    A, b = system(matrices, SYSTEMS[name][0])
    host = M is None
    M = block_object(matrices, SYSTEMS[name][0], blocks) if host else M
    thr = threshold(b, rtol)
    traj = trajectory(A, b, variant, M, max_iter - 1, thr=thr, key=(case[:5] if host else None))
    k_stop, status = stop_of(traj, thr)
    return A, b, thr, M, traj, k_stop, status


def stops_as_needed(case, traj, k_stop, status):
    max_iter, how = case[4], case[5]
    assert status in (CONVERGED, BREAKDOWN) and 0 < k_stop < max_iter - 6, (case_id(case), k_stop, status)
    assert how is None or status == how, (case_id(case), 'the oracle stops with status', status)
    assert k_stop > sum(CHUNKS), 'the stop must lie behind the short prcg_iterate calls'
    assert np.isfinite(traj['scalars'][:k_stop]).all() and np.isfinite(traj['coef'][:k_stop]).all()
    assert np.isfinite(traj['at'][k_stop]['x']).all(), 'x at the stop'


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_header_and_binding():
    from new_cg_variants_amd import _lib as L
    text = open(os.path.join(ROOT, 'include', 'prcg.h')).read()
    pub = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    assert re.search(r'\bint\s+prcg_set_stop_block_jacobi\s*\(\s*prcg_t\s*\*\s*h\s*,\s*const\s+double\s*\*\s*rr_stop\s*\)', pub)
    assert 'prcg_set_stop_block_jacobi' in L._SIGNATURES and hasattr(L.lib(), 'prcg_set_stop_block_jacobi')
    assert L.lib().prcg_version() == 1


def test_python_argument_checks_come_before_any_device_call(monkeypatch, matrices):
    import inspect

    import new_cg_variants_amd.callbacks as cbs
    import new_cg_variants_amd.cg_variants as cgv

    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(cgv, 'DeviceCSR', no_device)
    monkeypatch.setattr(cgv, '_operator', no_device)
    A, z = matrices['bcsstk03']
    b = np.asarray(z['b'], dtype=np.float64)
    n = A.shape[0]
    x0 = np.zeros(n)
    d = 1 / A.diagonal()
    served = [cgv.BlockJacobi(A, 2), cgv.DeviceBlockJacobi(A, 3), cgv.VarBlockJacobi(A, cyclic_partition(n)), cgv.DeviceVarBlockJacobi(A, cyclic_partition(n))]
    for name in BPCG:
        f = getattr(cgv, name)
        assert name in cgv.__all__
        assert list(inspect.signature(f).parameters)[:8] == ['A', 'b', 'x0', 'max_iter', 'preconditioner', 'callbacks', 'rtol', 'atol']
        # anything but a block-Jacobi object, with or without the keywords
        for prec, what in ((None, 'no preconditioner'), (cgv.Jacobi(A), 'a diagonal scaling'), (lambda v: d * v, 'a function'),
                           (lambda v: np.roll(v, 1), 'a function'), (d, 'a ndarray')):
            for kw in ({}, {'rtol': 1e-8}):
                with pytest.raises(ValueError, match=rf'{name}: {what}: the function takes BlockJacobi, DeviceBlockJacobi, VarBlockJacobi or '
                                                     rf'DeviceVarBlockJacobi; use {name[:-5]}_pcg'):
                    f(A, b, x0, 5, prec, **kw)
        M = served[0]
        for key in ('rtol', 'atol'):
            with pytest.raises(ValueError, match=rf'{name}: {key} must be one value or 1 values, one per system -- got shape \(2,\)'):
                f(A, b, x0, 5, M, **{key: [1e-8, 1e-8]})
            with pytest.raises(ValueError, match=rf'{name}: {key}\[0\] = nan: the value of system 0 must be finite and >= 0'):
                f(A, b, x0, 5, M, **{key: np.nan})
            with pytest.raises(ValueError, match=rf'{name}: {key}\[0\] = inf'):
                f(A, b, x0, 5, M, **{key: np.inf})
            with pytest.raises(ValueError, match=rf'{name}: {key}\[0\] = -1.0'):
                f(A, b, x0, 5, M, **{key: -1.0})
        with pytest.raises(ValueError, match=rf'{name}: b must have shape \({n},\)'):
            f(A, b[:-1], x0, 5, M, rtol=1e-8)
        with pytest.raises(ValueError, match=r'DeviceBlockJacobi: made for a matrix of 112 rows, the system has 111'):
            f(A[:-1, :-1].tocsr(), b[:-1], x0[:-1], 5, served[1], rtol=1e-8)
        # what IS served gets as far as the device: every block object, either keyword, both, zero, none
        for M in served:
            for kw in (dict(rtol=1e-8), dict(atol=[1e-3]), dict(rtol=1e-8, atol=1e-12), dict(rtol=0.0), {}):
                with pytest.raises(AssertionError, match='the device was reached'):
                    f(A, b, x0, 5, M, callbacks=[cbs.updated_residual_2_norm], **kw)
        # the functions that were there keep refusing the keywords with such an object
        g = getattr(cgv, name.replace('_bpcg', '_pcg'))
        with pytest.raises(ValueError, match=r'rtol= / atol= serve no preconditioner but a diagonal scaling.*stored-tilde schedule'):
            g(A, b, x0, 5, preconditioner=served[0], rtol=1e-8)


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_the_oracle_of_the_table_stops_inside_its_run(matrices, case):
    """every row of the table: the oracle stops strictly inside the run, the way the case needs it (breakdown rows: status 2 with a
    finite x at the stop).  Rows whose blocks the device builds run here with the host restatement of that build, which the GPU
    case replaces by the blocks read back."""
    _, _, _, _, traj, k_stop, status = oracle_of(matrices, case)
    print(f'{case_id(case)}: the oracle stops at k = {k_stop} with status {status}: mu, nu, rr = {traj["scalars"][k_stop, [0, 3, 4]]}')
    stops_as_needed(case, traj, k_stop, status)
    assert traj['scalars'].shape[0] == k_stop + 1 and set(traj['at']) == {k_stop}


@pytest.mark.parametrize('variant', ['PIPE_PR', 'PIPE_P_M'])
def test_the_model_tells_a_wrong_stop_from_a_right_one(matrices, variant):
    """bcsstk03 with blocks of 8, stopped at the k the rule fires at (rtol 1e-6).  A schedule that skips the pair launch of the stop
    iteration leaves u~ (and, where w is recomputed, w~) of iteration k - 1 behind; one that runs update k + 1 after the stop moves
    x, r, p and s: either changes bits of the stop state, so the GPU cases can tell them from the right one."""
    import oracle.ne_oracle as O
    from block_jacobi_stop_common import _dot
    A, b = system(matrices, 'bcsstk03')
    M = block_object(matrices, 'bcsstk03', 'bs8')
    thr = threshold(b, 1e-6)
    traj = trajectory(A, b, variant, M, 119, thr=thr)
    k_stop, status = stop_of(traj, thr)
    assert status == CONVERGED and 2 < k_stop < 113, (k_stop, status)
    right = traj['at'][k_stop]
    before = trajectory(A, b, variant, M, k_stop - 1)['at'][k_stop - 1]
    assert not np.array_equal(before['ut'], right['ut']), 'u~ of k - 1: a skipped pair launch would go unseen'
    if FLAVOUR[variant].startswith('pr'):
        assert not np.array_equal(before['wt'], right['wt']) and not np.array_equal(before['w'], right['w'])
    with np.errstate(all='ignore'):
        st = O.pipe_start(A, b, np.zeros(b.size), prec=M, dot=_dot)
        for _ in range(k_stop + 1):
            O.pipe_advance(A, st, flavour=FLAVOUR[variant], prec=M, dot=_dot, square=lambda q: q * q)
    for v in ('x', 'r', 'p', 's', 'rt', 'st'):
        assert not np.array_equal(getattr(st, v), right[v]), f'{v} after update k + 1: a late update would go unseen'


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def check_schedule(s, name, blocks):
    """the stored-tilde schedule with blocks, whatever n: not the one-launch iteration, not the one-workgroup solver"""
    family = SYSTEMS[name][2]
    assert not s['fused'] and not s['small'] and not s['comm'] and not s['xp_deferred'], s
    assert s['block_jacobi'] and s['block_jacobi_var'] == BLOCKS[blocks][0].startswith('bjv'), s
    assert s['window'] == (family == 'window') and s['sliced_rows'] == (family == 'sliced'), s


@pytest.mark.gpu
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_a_block_jacobi_session_stops_where_the_oracle_does(amd, matrices, case):
    """One session with rr_stop = (rtol ||b||)^2: prcg_iterate calls of 1, 2, 37 and the rest without a sync between them, one
    prcg_sync, everything read; then prcg_iterate(5), which must change nothing.  The launches behind the stop -- up to 90
    iterations of four launches each -- were all enqueued before the host knew: each must have returned at once."""
    name, blocks, variant, rtol, max_iter, _ = case
    L = amd['L']
    A, b = system(matrices, SYSTEMS[name][0])
    M = block_object(matrices, SYSTEMS[name][0], blocks)
    built = BLOCKS[blocks][0].endswith('_built')
    op = open_operator(amd, A, name)
    try:
        rec = run_session(L, op, variant, b, max_iter, threshold(b, rtol), CHUNKS, begin_keyword(blocks, M), then=5)
        read = (op.get_block_jacobi_var() if BLOCKS[blocks][0] == 'bjv_built' else op.get_block_jacobi()) if built else None
    finally:
        op.close()
    check_schedule(rec['schedule'], name, blocks)
    _, _, thr, _, traj, k_stop, status = oracle_of(matrices, case, with_blocks_read_back(A, blocks, M, read) if built else None)
    print(f'{case_id(case)}: thr = {thr!r}, the oracle stops at k = {k_stop} with status {status}; the device at {rec["stop"]}')
    stops_as_needed(case, traj, k_stop, status)
    holds_trajectory(rec, traj, k_stop, status, max_iter, case_id(case))
    assert same_reading(rec, rec['again']), 'prcg_iterate on a stopped session is a no-op'


@pytest.mark.gpu
@pytest.mark.parametrize('variant,blocks', [('PIPE_PR', 'bs3'), ('PIPE_P_M', 'built3')])
def test_a_threshold_at_the_initial_residual_stops_at_row_0(amd, matrices, variant, blocks):
    """rr_stop = r0.r0 exactly, from a nonzero x0: rr <= rr_stop on row 0 -- stopped at 0 as converged; x is x0, the state is the
    start-up's (its product and pair launch are plain), no row beyond 0 is written and every later launch is a no-op"""
    L = amd['L']
    A, b = system(matrices, 'fem16')
    M = block_object(matrices, 'fem16', blocks)
    x0 = np.random.default_rng(3).standard_normal(A.shape[0])
    r0 = b - A @ x0
    thr = float(device_dot(r0, r0))
    max_iter = 12
    op = open_operator(amd, A, 'fem16')
    try:
        rec = run_session(L, op, variant, b, max_iter, thr, (3, 4), begin_keyword(blocks, M), then=5, x0=x0)
    finally:
        op.close()
    check_schedule(rec['schedule'], 'fem16', blocks)
    traj = trajectory(A, b, variant, M, max_iter - 1, thr=thr, x0=x0)
    assert stop_of(traj, thr) == (0, CONVERGED) and traj['scalars'][0, 4] == thr
    holds_trajectory(rec, traj, 0, CONVERGED, max_iter, 'row 0')
    assert np.array_equal(rec['at']['x'], x0) and np.array_equal(rec['at']['r'], r0)
    assert same_reading(rec, rec['again'])


@pytest.fixture(scope='module')
def free_run(amd, matrices):
    """fem16 with blocks of 3, PIPE_PR, 40 iterations WITHOUT a threshold on a fresh handle: the reading two tests compare with"""
    L = amd['L']
    A, b = system(matrices, 'fem16')
    M = block_object(matrices, 'fem16', 'bs3')
    op = open_operator(amd, A, 'fem16')
    try:
        return run_session(L, op, 'PIPE_PR', b, 41, None, CHUNKS, begin_keyword('bs3', M))
    finally:
        op.close()


@pytest.mark.gpu
def test_a_threshold_that_never_fires_changes_no_bit(amd, matrices, free_run):
    """rr_stop = 0 on a run that neither reaches r = 0 nor breaks down: the stop forms of all four launches ran 40 times and every
    vector, scalar, coefficient and history entry is that of the session without a threshold"""
    L = amd['L']
    A, b = system(matrices, 'fem16')
    M = block_object(matrices, 'fem16', 'bs3')
    op = open_operator(amd, A, 'fem16')
    try:
        never = run_session(L, op, 'PIPE_PR', b, 41, 0.0, CHUNKS, begin_keyword('bs3', M))
    finally:
        op.close()
    check_schedule(never['schedule'], 'fem16', 'bs3')
    assert never['stop'] == (-1, 0) and never['k'] == 40 and free_run['stop'] == (-1, 0) and free_run['k'] == 40
    assert np.isfinite(free_run['scalars'][:, :5]).all() and (free_run['scalars'][:, [0, 3, 4]] > 0).all()
    assert same_reading(never, free_run)


@pytest.mark.gpu
def test_a_stopped_session_leaves_no_trace_on_the_handle(amd, matrices, free_run):
    """after a session that stopped (at rtol 1e-2, inside 40 iterations), a session without a threshold on the SAME handle equals
    the one on a fresh handle: the word, the threshold and the skipped launches leave nothing behind"""
    L = amd['L']
    A, b = system(matrices, 'fem16')
    M = block_object(matrices, 'fem16', 'bs3')
    op = open_operator(amd, A, 'fem16')
    try:
        thr = threshold(b, 1e-2)
        stopped = run_session(L, op, 'PIPE_PR', b, 41, thr, (1, 2), begin_keyword('bs3', M))
        after = run_session(L, op, 'PIPE_PR', b, 41, None, CHUNKS, begin_keyword('bs3', M))
    finally:
        op.close()
    traj = trajectory(A, b, 'PIPE_PR', M, 40, thr=thr)
    k_stop, status = stop_of(traj, thr)
    assert status == CONVERGED and 0 < k_stop < 34, (k_stop, status)
    holds_trajectory(stopped, traj, k_stop, status, 41, 'the stopped session')
    assert after['stop'] == (-1, 0) and same_reading(after, free_run)


@pytest.mark.gpu
def test_cg_variants_stop_at_rtol(amd, matrices):
    """pipe_pr_bpcg(..., BlockJacobi(A, 3), rtol=1e-8) on fem16: 'iterations', 'status' and the history are the oracle's; a foreign
    callback sees the states 0..k_stop and none after; x at the stop is the session's.  Without the keywords: pipe_pr_pcg's result."""
    import new_cg_variants_amd.callbacks as cbs
    cgv, L = amd['cgv'], amd['L']
    case = CASES[0]
    name, blocks, variant, rtol, max_iter, _ = case
    assert (name, blocks, variant) == ('fem16', 'bs3', 'PIPE_PR')
    A, b, thr, M, traj, k_stop, status = oracle_of(matrices, case)
    stops_as_needed(case, traj, k_stop, status)
    n = A.shape[0]
    op = open_operator(amd, A, name)
    try:
        rec = run_session(L, op, variant, b, max_iter, thr, (max_iter - 1,), begin_keyword(blocks, M))
    finally:
        op.close()
    holds_trajectory(rec, traj, k_stop, status, max_iter, 'the session')
    cgv.clear_operator_cache()
    try:
        seen = []

        def foreign(**env):
            seen.append((env['k'], float(env['nu_k']), env['x_k'].copy(), env['ut_k'].copy()))
        out = cgv.pipe_pr_bpcg(A, b, np.zeros(n), max_iter, M, callbacks=[cbs.updated_residual_2_norm, foreign], rtol=rtol)
        assert out['iterations'] == k_stop and out['status'] == 'converged'
        assert np.array_equal(out['updated_residual_2_norm'], rec['hist']) and not out['updated_residual_2_norm'][k_stop + 1:].any()
        assert [k for k, _, _, _ in seen] == list(range(k_stop + 1)), [k for k, _, _, _ in seen]
        assert [nu for _, nu, _, _ in seen] == traj['scalars'][:k_stop + 1, 3].tolist()
        assert np.array_equal(seen[-1][2], rec['at']['x']) and np.array_equal(seen[-1][3], rec['at']['ut'])
        # recorders only: one prcg_iterate call; the blocks built on the device; atol far above the initial residual
        out2 = cgv.pipe_pr_bpcg(A, b, np.zeros(n), max_iter, M, callbacks=[cbs.updated_residual_2_norm], rtol=rtol)
        assert out2['iterations'] == k_stop and out2['status'] == 'converged' and np.array_equal(out2['updated_residual_2_norm'], rec['hist'])
        out3 = cgv.pipe_p_m_bpcg(A, b, np.zeros(n), 12, cgv.DeviceBlockJacobi(A, 3), callbacks=[cbs.updated_residual_2_norm], atol=1e3 * np.linalg.norm(b))
        assert out3['iterations'] == 0 and out3['status'] == 'converged' and not out3['updated_residual_2_norm'][1:].any()
        out4 = cgv.pipe_pr_m_bpcg(A, b, np.zeros(n), 6, M, callbacks=[cbs.updated_residual_2_norm], rtol=1e-30)
        assert out4['iterations'] == 5 and out4['status'] == 'max_iter' and (out4['updated_residual_2_norm'] > 0).all()
        # without the keywords: no stop, no new keys -- pipe_pr_pcg with the same object, bit for bit
        plain = cgv.pipe_pr_pcg(A, b, np.zeros(n), 30, preconditioner=M, callbacks=[cbs.updated_residual_2_norm])
        same = cgv.pipe_pr_bpcg(A, b, np.zeros(n), 30, M, callbacks=[cbs.updated_residual_2_norm])
        assert 'iterations' not in same and 'status' not in same and set(same) == set(plain)
        assert np.array_equal(same['updated_residual_2_norm'], plain['updated_residual_2_norm']) and (same['updated_residual_2_norm'] > 0).all()
        # ... and a multi-RHS function on the cached operator is served afterwards: the threshold was the session's
        two = cgv.hs_bpcg_multi(A, np.stack([b, 2 * b]), np.zeros((2, n)), 5, M, callbacks=[cbs.updated_residual_2_norm])
        assert len(two) == 2
    finally:
        cgv.clear_operator_cache()


@pytest.mark.gpu
def test_what_the_threshold_does_not_serve_is_refused(amd, matrices):
    """through the C-ABI, each with its message naming the setter and how to clear it; nothing falls back"""
    L = amd['L']
    lib = L.lib()
    A, b = system(matrices, 'nos7')
    n = A.shape[0]
    x0 = np.zeros(n)
    inv_diag = 1 / A.diagonal()
    op = open_operator(amd, A, 'nos7')
    h = op._h
    k_stop, status = np.full(1, 7, dtype=np.int32), np.full(1, 7, dtype=np.int32)

    def error():
        return lib.prcg_last_error(h).decode()

    def begin(variant, d=None):
        return lib.prcg_solve_begin(h, variant, L.ptr(b), L.ptr(x0), 12, None, L.ptr(d), 1)

    def refused(rc, *words):
        text = error()
        assert rc == L.EINVAL, rc
        for w in ('prcg_set_stop_block_jacobi', 'prcg_set_stop_block_jacobi(h, NULL) clears the threshold') + words:
            assert w in text, (w, text)
    try:
        assert lib.prcg_get_stop(h, L.ptr(k_stop), L.ptr(status)) == L.EINVAL and 'prcg_get_stop: no open session' in error()
        assert k_stop[0] == status[0] == 7
        assert lib.prcg_set_stop_block_jacobi(None, L.ptr(np.array([1.0]))) == L.EINVAL
        good = np.array([1e-30])
        assert lib.prcg_set_stop_block_jacobi(h, L.ptr(good)) == L.OK
        for bad, text in ((np.nan, 'nan'), (np.inf, 'inf'), (-np.inf, '-inf'), (-1e-300, '-1e-300')):
            assert lib.prcg_set_stop_block_jacobi(h, L.ptr(np.array([bad]))) == L.EINVAL
            assert re.search(rf'prcg_set_stop_block_jacobi: rr_stop = {re.escape(text)}: the threshold must be finite and >= 0', error()), error()
        # (what was set before a bad value stays) no blocks in force: the text points to prcg_set_stop
        refused(begin(L.PIPE_PR), 'no blocks are in force', 'stops through prcg_set_stop ')
        assert lib.prcg_get_stop(h, L.ptr(k_stop), L.ptr(status)) == L.EINVAL          # (a refused begin opens nothing)
        op.build_block_jacobi(4)
        for variant in (L.HS, L.PR, L.M, L.CG_CG, L.GV):
            refused(begin(variant), 'which serves the pipelined variants', f'variant {variant} is not pipelined')
        refused(begin(L.PIPE_PR, inv_diag), 'inv_diag overrides the blocks')
        hook = L.REPLACE_FN(lambda ctx, k: 0)
        assert lib.prcg_set_replace_hook(h, C.cast(hook, C.c_void_p), None) == L.OK
        refused(begin(L.PIPE_P), 'a replace hook is set')
        assert lib.prcg_set_replace_hook(h, None, None) == L.OK
        # the multi-RHS begins
        B, X0 = np.stack([b, b]), np.zeros((2, n))
        cols, zeros = amd['device']._row_pointers(B), amd['device']._row_pointers(X0)
        refused(lib.prcg_solve_begin_multi_block_jacobi(h, L.HS, 2, cols, zeros, 12, 1), 'prcg_solve_begin_multi_block_jacobi', 'SINGLE sessions')
        op.set_block_jacobi(0, None)           # (the sessions without blocks refuse a handle that holds some with a text of their own)
        refused(lib.prcg_solve_begin_multi(h, L.HS, 2, cols, zeros, 12, L.ptr(inv_diag), 1), 'prcg_solve_begin_multi:')
        refused(lib.prcg_solve_begin_multi_pipe(h, L.PIPE_PR, 2, cols, zeros, 12, L.ptr(inv_diag), 1), 'prcg_solve_begin_multi_pipe:')
        op.build_block_jacobi(4)
        # with prcg_set_stop set as well, its refusal of a session with blocks stands
        assert lib.prcg_set_stop(h, L.ptr(good)) == L.OK
        assert begin(L.PIPE_PR) == L.EINVAL and 'a stop threshold is set (prcg_set_stop)' in error() and 'block-Jacobi preconditioner is in force' in error()
        assert lib.prcg_set_stop(h, None) == L.OK
        # a host callback replaces the blocks: refused, whichever of the two the text names
        fn = L.PREC_FN(lambda ctx, count, v, out: 1)
        assert lib.prcg_set_preconditioner(h, C.cast(fn, C.c_void_p), None) == L.OK
        refused(begin(L.PIPE_PR_M), 'a host-callback preconditioner is in force')
        assert lib.prcg_set_preconditioner(h, None, None) == L.OK
        op.build_block_jacobi(4)
        # served: every pipelined variant; running -> {-1, 0}; the state is not set from outside
        for variant in (L.PIPE_PR, L.PIPE_PR_M, L.PIPE_P, L.PIPE_P_M):
            assert begin(variant) == L.OK, error()
            assert lib.prcg_get_stop(h, L.ptr(k_stop), L.ptr(status)) == L.OK and (k_stop[0], status[0]) == (-1, 0)
            s = op.schedule()
            assert s['block_jacobi'] and not s['fused'] and not s['small'], s
        assert lib.prcg_get_stop(h, None, L.ptr(status)) == L.EINVAL and 'null buffer' in error()
        row = np.zeros(8)
        for call, who in ((lambda: lib.prcg_set_vector(h, L.VEC['x'], L.ptr(x0)), 'prcg_set_vector'),
                          (lambda: lib.prcg_set_scalars(h, 0, L.ptr(row)), 'prcg_set_scalars'), (lambda: lib.prcg_set_iteration(h, 0), 'prcg_set_iteration')):
            assert call() == L.EINVAL and f'{who}: the open session was begun with a stop threshold' in error(), (who, error())
        # a null clear: everything is served again, a session has no stop, the setters work
        assert lib.prcg_set_stop_block_jacobi(h, None) == L.OK
        assert begin(L.HS) == L.OK
        assert lib.prcg_get_stop(h, L.ptr(k_stop), L.ptr(status)) == L.OK and (k_stop[0], status[0]) == (-1, 0)
        assert lib.prcg_set_vector(h, L.VEC['x'], L.ptr(x0)) == L.OK
        assert lib.prcg_solve_begin_multi_block_jacobi(h, L.HS, 2, cols, zeros, 12, 1) == L.OK, error()
    finally:
        op.close()
    # DeviceCSR.begin routes the threshold by the blocks and leaves none behind
    op = open_operator(amd, A, 'nos7')
    try:
        op.begin(L.PIPE_PR, b, x0, 12, block_jacobi=(4, None), rr_stop=1e300)
        assert op.stop() == (0, CONVERGED)
        op.begin(L.PIPE_PR, b, x0, 12, inv_diag=inv_diag, rr_stop=1e300)          # (prcg_set_stop's session; the blocks stay, overridden)
        assert op.stop() == (0, CONVERGED) and op.schedule()['fused']
        with pytest.raises(L.PrcgError, match='variant 0 is not pipelined'):
            op.begin(L.HS, b, x0, 12, block_jacobi=(4, None), rr_stop=1.0)
        op.begin(L.HS, b, x0, 12, block_jacobi=(4, None))
        assert op.stop() == (-1, 0)
        op.begin_multi_block_jacobi(L.HS, np.stack([b, b]), np.zeros((2, n)), 12, block_jacobi=(4, None))
    finally:
        op.close()
