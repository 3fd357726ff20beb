"""CPU: what tests/test_hs_stop.py assumes about its cases, and the host side of the Hestenes-Stiefel stop (prcg.h: prcg_set_stop_hs;
cg_variants.hs_cg_stop / hs_pcg_stop).

The cases of hs_stop_common.CASES were chosen with the oracle under np.dot; the GPU test asserts the same conditions again under the
device's summation order.  Here, for every case: thr = rr at max_iter // 2 gives an interior stop with status 1 (at max_iter // 2,
except bcsstk03, whose residual is not monotone: 16 of 40); thr = 0 never fires; the indefinite operators break down where the
GPU test expects (status 2, mu < 0, k = 19 / 14).  And the rule is THE rule: one that ignores mu, or that looks at row k + 1 where
it should look at row k, stops somewhere else."""
import os
import re

import numpy as np
import pytest

from hs_stop_common import BREAKDOWN, BREAKDOWNS, CASES, CONVERGED, case_id, make_problem, rule, stop_of, trajectory_np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def problem(matrices):
    from new_cg_variants_amd import problems
    return make_problem(problems, matrices)


def stop_ignoring_mu(traj, thr):
    for k, (_, _, _, nu, rr) in enumerate(traj['scalars']):
        status = rule(1.0, nu, rr, thr)
        if status:
            return k, status
    return -1, 0


def stop_one_row_late(traj, thr):
    """the rule applied to row k + 1 where the launch should apply it to row k: the session would hold the state of k"""
    rows = traj['scalars']
    for k in range(len(rows) - 1):
        status = rule(rows[k + 1][0], rows[k + 1][3], rows[k + 1][4], thr)
        if status:
            return k, status
    return -1, 0


@pytest.mark.parametrize('operator,method,max_iter', CASES, ids=[case_id(c) for c in CASES])
def test_the_cases_stop_inside_their_run(problem, operator, method, max_iter):
    A, b, _ = problem(operator)
    traj = trajectory_np(A, b, method, max_iter - 1, keep=())
    thr = float(traj['scalars'][max_iter // 2, 4])
    k_stop, status = stop_of(traj, thr)
    assert np.isfinite(thr) and thr > 0 and status == CONVERGED and 0 < k_stop < max_iter - 1, (thr, k_stop, status)
    assert k_stop == (16 if operator == 'bcsstk03_wg' else max_iter // 2), k_stop
    assert np.isfinite(traj['scalars']).all() and stop_of(traj, 0.0) == (-1, 0), 'thr = 0 never fires on a run that does not break down'
    assert stop_one_row_late(traj, thr) == (k_stop - 1, CONVERGED), 'a rule on row k + 1 stops one iteration early'
    assert stop_ignoring_mu(traj, thr) == (k_stop, CONVERGED)      # (mu matters at a breakdown only: below)


@pytest.mark.parametrize('operator,method,max_iter,k_break', BREAKDOWNS, ids=[case_id(c) for c in BREAKDOWNS])
def test_the_indefinite_operators_break_down(problem, operator, method, max_iter, k_break):
    A, b, _ = problem(operator)
    traj = trajectory_np(A, b, method, max_iter - 1)
    k_stop, status = stop_of(traj, 1e-300)
    mu, _, _, nu, rr = traj['scalars'][k_stop]
    assert (k_stop, status) == (k_break, BREAKDOWN) and mu < 0 < nu and rr > 1e-300, (k_stop, status, mu, nu, rr)
    assert np.isfinite(traj['scalars'][:k_stop + 1]).all() and np.isfinite(traj['at'][k_stop]['x']).all()
    assert stop_ignoring_mu(traj, 1e-300) != (k_stop, status), 'a rule that ignores mu runs past the breakdown'
    assert stop_one_row_late(traj, 1e-300) == (k_stop - 1, BREAKDOWN)


def test_header_and_binding():
    from new_cg_variants_amd import _lib as L
    text = open(os.path.join(ROOT, 'include', 'prcg.h')).read()
    pub = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = L.lib()
    assert re.search(r'\bint\s+prcg_set_stop_hs\s*\(\s*prcg_t\s*\*\s*h\s*,\s*const\s+double\s*\*\s*rr_stop\s*\)\s*;', pub)
    assert 'prcg_set_stop_hs' in L._SIGNATURES and hasattr(lib, 'prcg_set_stop_hs')
    assert lib.prcg_version() == 1
    section = text[text.index('a single HESTENES-STIEFEL session stopped at a residual threshold'):text.index('each column of a PIPELINED TWO-RHS session')]
    for word in ('prcg_set_stop_hs', 'rr <= *rr_stop', 'breakdown', 'converged', 'NULL clears', 'PRCG_FUSED=0', 'replace hook', 'stored-tilde',
                 'one product per solve', 'prcg_set_vector, prcg_set_scalars and prcg_set_iteration', 'prcg_solve_begin_multi'):
        assert word in section, word


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
    assert 'hs_cg_stop' in cgv.__all__ and 'hs_pcg_stop' in cgv.__all__
    for name in ('hs_cg_stop', 'hs_pcg_stop'):
        f = getattr(cgv, name)
        assert f.__name__ == name and [q for q in ('rtol', 'atol') if inspect.signature(f).parameters[q].default is None] == ['rtol', 'atol']
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
        # what IS served gets as far as the device: either keyword, both, zero, none
        for kw in (dict(rtol=1e-8), dict(atol=[1e-3]), dict(rtol=1e-8, atol=1e-12), dict(rtol=0.0), {}):
            with pytest.raises(AssertionError, match='the device was reached'):
                f(A, b, x0, 5, callbacks=[cbs.updated_residual_2_norm], **kw)
    d = 1 / A.diagonal()
    for prec in (None, cgv.Jacobi(A), lambda v: d * v):
        with pytest.raises(AssertionError, match='the device was reached'):
            cgv.hs_pcg_stop(A, b, x0, 5, preconditioner=prec, rtol=1e-8)
    # a preconditioner that is no diagonal scaling runs the schedule with reduction launches: refused here, with or without the keywords
    for prec in (cgv.BlockJacobi(A, 2), lambda v: np.roll(v, 1)):
        for kw in (dict(rtol=1e-8), {}):
            with pytest.raises(ValueError, match=r'hs_pcg_stop: the function takes no preconditioner but a diagonal scaling.*use hs_pcg'):
                cgv.hs_pcg_stop(A, b, x0, 5, preconditioner=prec, **kw)
    # hs_cg / hs_pcg themselves never took the keywords and keep passing them by, whatever their value: unchanged
    for name in ('hs_cg', 'hs_pcg'):
        with pytest.raises(AssertionError, match='the device was reached'):
            getattr(cgv, name)(A, b, x0, 5, rtol=-1.0)
        assert name + '_stop' in getattr(cgv, name).__doc__
    with pytest.raises(AssertionError, match='the device was reached'):
        cgv.hs_pcg(A, b, x0, 5, preconditioner=cgv.BlockJacobi(A, 2), rtol=1e-8)
