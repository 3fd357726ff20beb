"""Every system of a batch stops at its OWN residual threshold, decided inside its workgroup (prcg.h: prcg_batch_set_stop,
prcg_batch_get_stops; device.DeviceBatch.begin(rr_stop=...), .stops(); cg_variants.*_batch(rtol=, atol=)).

The rule, on row k of a system's scalars (mu = [0], nu = [3], rr = [4]) after iteration k and at k = 0 on the initial state:
rr <= thr -> converged (1); else !(0 < mu < inf and 0 < nu < inf) -> breakdown (2); else go on.  A stopped system keeps the
complete state of its stop iteration, rows beyond stay zero, later launches leave it alone.

The reference is oracle/ne_oracle.py stepped under the workgroup's sum (wg_dot) with the rule applied in Python to its own mu,
nu and wg_dot(r, r); every comparison is np.array_equal -- there is no tolerance in this file.

CPU: header and binding; the Python argument checks; and the INPUTS: the oracle alone must show the mix of stops (k = 1, never,
five or more distinct iterations, breakdown before convergence, both entry cases) that makes a GPU pass mean something.
GPU: the stopped run of the nine systems against the oracle; cutting; a threshold never met against the plain session; order
and company; 300 systems with per-system thresholds; the entry rule and isolation; breakdown caught before the NaNs; the C-ABI's
refusals; the public functions."""
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
from small_batch_common import (BREAKDOWN, CONVERGED, NINE, VARIANTS, holds_oracle, jacobi_of, oracle_stopped, rule, run_stopping_batch, system,
                                thresholds)

ITERS = 150
RTOL = 1e-8
NAMES = [name for name, _, _ in NINE]


def indefinite():
    """A = diag(+1 x 32, -1 x 32), b = ones: mu = p.s = 0 on the initial state, with the Jacobi scaling (d = +-1: nu = 0 too) and
    without -- a breakdown at k = 0"""
    return sp.csr_matrix(sp.diags(np.concatenate([np.ones(32), -np.ones(32)]))), np.ones(64)


@pytest.fixture(scope='module')
def nine(matrices):
    return [system(matrices, name) for name in NAMES]


@pytest.fixture(scope='module')
def special(matrices):
    A4, b4 = system(matrices, 'nos4')
    return {'indefinite': indefinite(), 'nos4_b0': (A4, np.zeros(b4.size))}


@pytest.fixture(scope='module')
def oracle(matrices, nine, special):
    """(system name, variant, thr, iters, jacobi) -> oracle_stopped of it: computed once, never modified"""
    cache = {}
    systems = dict(zip(NAMES, nine), **special)

    def get(name, variant, thr, iters=ITERS, jacobi=True):
        key = (name, variant, float(thr), iters, jacobi)
        if key not in cache:
            A, b = systems[name]
            cache[key] = oracle_stopped(A, b, variant, float(thr), iters, jacobi)
        return cache[key]
    return get


@pytest.fixture(scope='module')
def nine_thr(nine):
    return thresholds([b for _, b in nine], rtol=RTOL)


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_header_and_binding():
    from new_cg_variants_amd import _lib as L
    text = open(os.path.join(ROOT, 'include', 'prcg.h')).read()
    pub = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    lib = L.lib()
    for name in ('prcg_batch_set_stop', 'prcg_batch_get_stops'):
        assert re.search(rf'\b{name}\s*\(', pub), name
        assert name in L._SIGNATURES and hasattr(lib, name), name
    assert lib.prcg_version() == 1
    section = text[text.index('a BATCH of small independent systems'):text.index('typedef struct prcg_batch')]
    for word in ('prcg_batch_set_stop', 'prcg_batch_get_stops', 'rr <= rr_stop[s]', 'breakdown', 'converged', 'NULL clears'):
        assert word in section, word


def test_python_argument_checks_come_before_any_device_call(monkeypatch, matrices):
    import new_cg_variants_amd.callbacks as cbs
    import new_cg_variants_amd.cg_variants as cgv
    from new_cg_variants_amd import device

    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(cgv, 'DeviceBatch', no_device)
    monkeypatch.setattr(cgv, 'DeviceCSR', no_device)
    monkeypatch.setattr(cgv, '_operator', no_device)
    A, b = system(matrices, 'bcsstk03')
    n = A.shape[0]
    bs, x0s = [b, 2 * b, 3 * b], [np.zeros(n)] * 3
    for name in ('pipe_pr_cg_batch', 'pipe_pr_m_cg_batch', 'hs_cg_batch', 'pipe_pr_pcg_batch', 'pipe_pr_m_pcg_batch', 'hs_pcg_batch'):
        f = getattr(cgv, name)
        for key in ('rtol', 'atol'):
            with pytest.raises(ValueError, match=rf'{name}: {key} must be one value or 3 values, one per system -- got shape \(2,\)'):
                f(A, bs, x0s, 5, **{key: [1e-8, 1e-8]})
            with pytest.raises(ValueError, match=rf'{name}: {key}\[1\] = nan: the value of system 1 must be finite and >= 0'):
                f(A, bs, x0s, 5, **{key: [1e-8, np.nan, 1e-8]})
            with pytest.raises(ValueError, match=rf'{name}: {key}\[2\] = -1e-08: the value of system 2'):
                f(A, bs, x0s, 5, **{key: [0.0, 1e-8, -1e-8]})
            with pytest.raises(ValueError, match=rf'{name}: {key}\[0\] = inf'):
                f(A, bs, x0s, 5, **{key: np.inf})
            with pytest.raises(ValueError, match=rf'{name}: {key}\[0\] = -1.0'):
                f(A, bs, x0s, 5, **{key: -1.0})
        # what IS served gets as far as the device: a scalar, one value per system, both, zero
        for kw in (dict(rtol=1e-8), dict(atol=[1e-3, 0.0, 1.0]), dict(rtol=np.full(3, 1e-8), atol=1e-12), dict(rtol=0.0)):
            with pytest.raises(AssertionError, match='the device was reached'):
                f(A, bs, x0s, 5, callbacks=[cbs.updated_residual_2_norm], **kw)
    # DeviceBatch.begin shapes rr_stop with batch_thresholds: a scalar for all, or one value per system
    assert device.batch_thresholds('rr_stop', 0.25, 3).tolist() == [0.25] * 3
    assert device.batch_thresholds('rr_stop', [0, 1e-300, 1e300], 3).tolist() == [0.0, 1e-300, 1e300]
    with pytest.raises(ValueError, match=r'rr_stop must be one value or 3 values, one per system -- got shape \(4,\)'):
        device.batch_thresholds('rr_stop', np.ones(4), 3)
    with pytest.raises(ValueError, match=r'rr_stop\[2\] = nan: the value of system 2 must be finite and >= 0'):
        device.batch_thresholds('rr_stop', [1.0, 0.0, np.nan], 3)
    with pytest.raises(ValueError, match=r'rr_stop\[0\] = -0.5'):
        device.batch_thresholds('rr_stop', -0.5, 3)
    with pytest.raises(ValueError, match=r'rr_stop\[1\] = inf'):
        device.batch_thresholds('rr_stop', [1.0, np.inf, 1.0], 3)
    import inspect
    assert inspect.signature(device.DeviceBatch.begin).parameters['rr_stop'].default is None
    # ... and begin checks it before it touches the library
    batch = object.__new__(device.DeviceBatch)
    batch.sizes, batch.n_sys = [n, n], 2

    class NoLib:
        def __getattr__(self, name):
            raise AssertionError('the device was reached')
    batch._lib, batch._h, batch._b = NoLib(), None, None
    for bad in ([1.0], [1.0, np.nan], [-1.0, 1.0], np.inf):
        with pytest.raises(ValueError, match='rr_stop'):
            batch.begin(0, [b, b], [np.zeros(n)] * 2, 5, rr_stop=bad)
    with pytest.raises(AssertionError, match='the device was reached'):
        batch.begin(0, [b, b], [np.zeros(n)] * 2, 5, rr_stop=[1.0, 0.0])


@pytest.mark.parametrize('variant', VARIANTS)
def test_the_oracle_alone_shows_the_mix_of_stops(nine, oracle, nine_thr, variant):
    """nine systems, Jacobi, rtol = 1e-8, 150 iterations: the stop iterations are derived here, not hard-coded (measured:
    PIPE_PR 134, 77, 1, 97, 59, -1, 70, 74, 75; PIPE_PR_M 133, 77, 1, 97, 59, -1, 71, 74, 75; HS 129, 77, 1, 99, 59, -1, 65, 74, 75)"""
    runs = [oracle(name, variant, thr) for name, thr in zip(NAMES, nine_thr)]
    stops = [r['k_stop'] for r in runs]
    print(variant, stops, [r['status'] for r in runs])
    assert 1 in stops, 'one system stops at k = 1'
    assert -1 in stops, 'one system is still running at 150'
    assert len({k for k in stops if k >= 0}) >= 5, 'at least five distinct stop iterations'
    for name, r in zip(NAMES, runs):
        assert r['status'] in (0, CONVERGED) and (r['k_stop'] >= 0) == (r['status'] == CONVERGED), name
        assert r['last'] == (r['k_stop'] if r['status'] else ITERS) and r['scalars'].shape == (r['last'] + 1, 5), name
        if r['status']:
            assert np.all(np.isfinite(r['at']['x'])), name
            assert r['scalars'][-1, 4] <= nine_thr[NAMES.index(name)] < r['scalars'][-2, 4], name


@pytest.mark.parametrize('variant', ['PIPE_PR', 'PIPE_PR_M'])
def test_the_oracle_shows_breakdown_before_convergence(nine, oracle, variant):
    """nos7, Jacobi, rtol = 1e-10: the pipelined recurrences break down (measured: k = 104 PIPE_PR, 103 PIPE_PR_M) before the
    residual gets there, with a finite x"""
    A, b = nine[NAMES.index('nos7')]
    thr = thresholds([b], rtol=1e-10)[0]
    r = oracle('nos7', variant, thr)
    print(variant, r['k_stop'], r['status'])
    assert r['status'] == BREAKDOWN and 1 <= r['k_stop'] < ITERS
    assert np.all(r['scalars'][:, 4] > thr), 'no convergence before the breakdown'
    mu, nu = r['scalars'][-1, 0], r['scalars'][-1, 3]
    assert not (0 < mu < np.inf and 0 < nu < np.inf)
    assert np.all(np.isfinite(r['at']['x']))
    # every earlier row passes the rule: the stop is the FIRST breakdown
    assert all(rule(row[0], row[3], row[4], thr) == 0 for row in r['scalars'][:-1])


@pytest.mark.parametrize('jacobi', [True, False])
@pytest.mark.parametrize('variant', VARIANTS)
def test_the_oracle_shows_both_entry_cases(oracle, variant, jacobi):
    r = oracle('indefinite', variant, thresholds([np.ones(64)], rtol=RTOL)[0], jacobi=jacobi)
    assert (r['k_stop'], r['status'], r['last']) == (0, BREAKDOWN, 0) and r['scalars'][0, 4] == 64.0 and r['scalars'][0, 0] == 0.0
    r = oracle('nos4_b0', variant, 0.0, jacobi=jacobi)
    assert (r['k_stop'], r['status'], r['last']) == (0, CONVERGED, 0) and r['scalars'][0, 4] == 0.0 and r['scalars'][0, 0] == 0.0
    assert np.array_equal(r['at']['x'], np.zeros(100))


@pytest.mark.parametrize('variant', VARIANTS)
def test_the_oracle_shows_a_zero_threshold_never_met(oracle, variant):
    """unpreconditioned, 60 iterations, thr = 0: the rule never fires; nor in 10 Jacobi iterations without bcsstm22"""
    for name in NAMES:
        r = oracle(name, variant, 0.0, iters=60, jacobi=False)
        assert (r['k_stop'], r['status'], r['last']) == (-1, 0, 60), name
        if name != 'bcsstm22':
            r = oracle(name, variant, 0.0, iters=10)
            assert (r['k_stop'], r['status'], r['last']) == (-1, 0, 10), name


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def amd():
    import new_cg_variants_amd.callbacks as cbs
    import new_cg_variants_amd.cg_variants as cgv
    from new_cg_variants_amd import _lib, device, problems
    return dict(cgv=cgv, cbs=cbs, L=_lib, device=device, problems=problems)


def run_batch(amd, systems, variant, rr_stop, chunks=(ITERS,), **kw):
    return run_stopping_batch(amd, systems, variant, rr_stop, chunks, **kw)


def same(a, b, what=''):
    """two device records, whole"""
    assert (a['k_stop'], a['status']) == (b['k_stop'], b['status']), (what, 'stop word')
    for key in ('at0', 'at'):
        assert a[key].keys() == b[key].keys()
        for v in a[key]:
            assert np.array_equal(a[key][v], b[key][v], equal_nan=True), (what, key, v)
    for key in ('scalars', 'coef', 'hist'):
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key], equal_nan=True), (what, key)


@pytest.fixture(scope='module')
def base(amd, nine, nine_thr):
    """variant -> the records of the nine systems, Jacobi, rtol = 1e-8, 150 iterations in ONE call: computed once, never modified"""
    cache = {}

    def get(variant):
        if variant not in cache:
            cache[variant] = run_batch(amd, nine, variant, nine_thr)
        return cache[variant]
    return get


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_whole_stopped_run_against_the_oracle(nine, oracle, nine_thr, base, variant):
    for name, thr, rec in zip(NAMES, nine_thr, base(variant)):
        holds_oracle(rec, oracle(name, variant, thr), variant, ITERS, name)
    assert base(variant)[NAMES.index('494_bus')]['k_stop'] == -1     # ... whose vectors were compared at k = 150


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_cutting_changes_nothing(amd, nine, nine_thr, base, variant):
    """(1, 6, 1, 142): bcsstm22 stops on the first chunk's last iteration and is relaunched three times while stopped"""
    cut = run_batch(amd, nine, variant, nine_thr, chunks=(1, 6, 1, 142))
    assert base(variant)[NAMES.index('bcsstm22')]['k_stop'] == 1
    for name, a, b in zip(NAMES, cut, base(variant)):
        same(a, b, 'cut ' + name)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_a_threshold_never_met_is_the_plain_session(amd, nine, variant):
    """rr_stop = 0 where the oracle shows no stop: the STOP form of the bodies carries the bits of the existing kernels"""
    rest = [q for name, q in zip(NAMES, nine) if name != 'bcsstm22']
    for systems, iters, jacobi in ((nine, 60, False), (rest, 10, True)):
        stop = run_batch(amd, systems, variant, 0.0, chunks=(iters,), jacobi=jacobi)
        plain = run_batch(amd, systems, variant, None, chunks=(iters,), jacobi=jacobi)
        for i, (a, b) in enumerate(zip(stop, plain)):
            same(a, b, f'jacobi={jacobi} system {i}')
            assert (a['k_stop'], a['status']) == (-1, 0)
            assert np.all(np.isfinite(a['hist'])) and a['hist'][iters] > 0      # agreement of NaNs or zeros cannot carry the test


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_company_and_order(amd, nine, nine_thr, base, variant):
    want = base(variant)
    rev = run_batch(amd, nine[::-1], variant, nine_thr[::-1])[::-1]
    for name, a, b in zip(NAMES, rev, want):
        same(a, b, 'reversed ' + name)
    for i in (NAMES.index('nos7'), NAMES.index('lap40x40')):     # matrix in registers, matrix in LDS
        assert NINE[i][2] == (1 if NAMES[i] == 'nos7' else 0)
        alone = run_batch(amd, [nine[i]], variant, nine_thr[i:i + 1])
        same(alone[0], want[i], 'alone: ' + NAMES[i])


@pytest.mark.gpu
def test_more_systems_than_cus_with_per_system_thresholds(amd, matrices):
    A, b = system(matrices, 'nos4')
    n_sys, picked = 300, [0, 1, 150, 299]
    systems = [(A, b * (1 + s / 300)) for s in range(n_sys)]
    rtol = np.where(np.arange(n_sys) % 2 == 0, 1e-4, 1e-8)
    thr = thresholds([q for _, q in systems], rtol=rtol)
    L = amd['L']
    batch = amd['device'].DeviceBatch([A], np.zeros(n_sys, dtype=np.int32))
    try:
        batch.begin(L.PIPE_PR, [q for _, q in systems], np.zeros((n_sys, b.size)), ITERS + 1, hist_mask=1,
                    inv_diag=[1 / A.diagonal()] * n_sys, rr_stop=thr)
        batch.iterate(ITERS)
        k_stop, status = batch.stops()
        hists = np.array([batch.history(s)['updated_residual_2_norm'] for s in range(n_sys)])
        rr = np.array([[batch.get_scalars(k, s)[4] for k in (k_stop[s] - 1, k_stop[s])] for s in range(n_sys)])
    finally:
        batch.close()
    assert np.all(status == CONVERGED) and np.all(k_stop >= 1)
    assert k_stop[0::2].max() < k_stop[1::2].min()               # the looser tolerance stops earlier
    for s in range(n_sys):
        k = k_stop[s]
        assert rr[s, 1] <= thr[s] < rr[s, 0], s                  # the rule, on the scalars it reads
        assert hists[s, k] ** 2 <= thr[s] < hists[s, k - 1] ** 2, s
        assert np.all(hists[s, :k + 1] > 0) and np.array_equal(hists[s, k + 1:], np.zeros(ITERS - k)), s
    whole = run_batch(amd, systems, 'PIPE_PR', thr, mat_of=np.zeros(n_sys, dtype=np.int32), matrices=[A], read=picked)
    four = run_batch(amd, [systems[s] for s in picked], 'PIPE_PR', thr[picked], mat_of=np.zeros(4, dtype=np.int32), matrices=[A])
    for s, a, c in zip(picked, whole, four):
        same(a, c, f'system {s}')
        assert a['k_stop'] == k_stop[s] and np.array_equal(a['hist'], hists[s])


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_entry_rule_and_isolation(amd, nine, special, oracle, variant):
    iters = 60
    systems = [nine[NAMES.index('bcsstk03')], special['indefinite'], special['nos4_b0'], nine[NAMES.index('494_bus')]]
    thr = thresholds([b for _, b in systems], rtol=RTOL)
    assert thr[2] == 0.0 and thr[1] > 0
    got = run_batch(amd, systems, variant, thr, chunks=(iters,))
    holds_oracle(got[1], oracle('indefinite', variant, thr[1]), variant, iters, 'indefinite')
    holds_oracle(got[2], oracle('nos4_b0', variant, 0.0), variant, iters, 'b = 0')
    assert (got[1]['k_stop'], got[1]['status']) == (0, BREAKDOWN) and (got[2]['k_stop'], got[2]['status']) == (0, CONVERGED)
    for s in (1, 2):                                             # the k = 0 state untouched, and no NaN anywhere
        for v in got[s]['at']:
            assert np.array_equal(got[s]['at'][v], got[s]['at0'][v]) and np.all(np.isfinite(got[s]['at'][v])), (s, v)
        assert np.all(np.isfinite(got[s]['scalars'])) and np.all(np.isfinite(got[s]['coef'])) and np.all(np.isfinite(got[s]['hist']))
    assert np.array_equal(got[2]['at']['x'], np.zeros(100))      # x = x0
    for s in (0, 3):
        solo = run_batch(amd, [systems[s]], variant, thr[s:s + 1], chunks=(iters,))
        same(got[s], solo[0], f'system {s} against its solo run')
        assert np.all(np.isfinite(got[s]['hist'])) and got[s]['hist'][got[s]['k_stop'] if got[s]['status'] else iters] > 0


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['PIPE_PR', 'PIPE_PR_M'])
def test_breakdown_is_caught_before_the_nans(amd, nine, oracle, variant):
    i = NAMES.index('nos7')
    thr = thresholds([nine[i][1]], rtol=1e-10)
    want = oracle('nos7', variant, thr[0])
    got = run_batch(amd, [nine[i]], variant, thr)[0]
    holds_oracle(got, want, variant, ITERS, 'nos7')
    assert got['status'] == BREAKDOWN and np.all(np.isfinite(got['at']['x']))
    plain = run_batch(amd, [nine[i]], variant, None)[0]
    assert (plain['k_stop'], plain['status']) == (-1, 0)
    assert not np.all(np.isfinite(plain['at']['x'])), 'without thresholds the same session runs on into inf / nan'


@pytest.mark.gpu
def test_refusals_through_the_c_abi(amd, nine, oracle):
    L = amd['L']
    lib = L.lib()
    systems = [nine[NAMES.index('bcsstk03')], nine[NAMES.index('nos4')], nine[NAMES.index('model_48_8_3')]]
    rhs = np.concatenate([b for _, b in systems])
    x0, dinv = np.zeros(rhs.size), np.concatenate(jacobi_of(systems))
    batch = amd['device'].DeviceBatch([A for A, _ in systems])
    bt, h = batch._b, batch._h

    def error():
        return (lib.prcg_last_error(h) or b'').decode()

    def stops():
        k_stop, status = np.full(3, 7, dtype=np.int32), np.full(3, 7, dtype=np.int32)
        return lib.prcg_batch_get_stops(bt, L.ptr(k_stop), L.ptr(status)), k_stop.tolist(), status.tolist()

    def record(iters=10):
        assert lib.prcg_batch_iterate(bt, iters) == L.OK and lib.prcg_batch_sync(bt) == L.OK
        return ([batch.get_vector(v, 0) for v in ('x', 'r', 'p', 's')], np.array([batch.get_scalars(k, 0) for k in range(iters + 1)]),
                np.array([batch.get_coefficients(k, 0) for k in range(1, iters + 1)]))
    try:
        rc, k_stop, status = stops()
        assert rc == L.EINVAL and 'prcg_batch_get_stops: no open session' in error() and k_stop == status == [7] * 3
        thr0 = thresholds([systems[0][1]], rtol=1e-3)[0]
        want = oracle('bcsstk03', 'PIPE_PR', thr0, iters=60)
        assert want['status'] == CONVERGED and want['k_stop'] >= 1, 'the input: system 0 converges to 1e-3 ||b|| within 60 iterations'
        good = np.array([thr0, 0.0, 0.0])
        assert lib.prcg_batch_set_stop(bt, L.ptr(good)) == L.OK
        for s, bad, text in ((1, np.nan, 'nan'), (2, -1e-30, '-1e-30'), (0, np.inf, 'inf'), (2, -np.inf, '-inf')):
            arr = good.copy()
            arr[s] = bad
            assert lib.prcg_batch_set_stop(bt, L.ptr(arr)) == L.EINVAL
            assert re.search(rf'prcg_batch_set_stop: rr_stop\[{s}\] = {re.escape(text)}: the threshold of system {s} must be finite and >= 0',
                             error()), error()
        # the thresholds were copied at the call (the caller's buffer is theirs again), and a refusal left them alone
        good[:] = np.nan
        assert lib.prcg_batch_begin_jacobi(bt, L.PIPE_PR, L.ptr(rhs), L.ptr(x0), L.ptr(dinv), 61, 1) == L.OK
        rc, k_stop, status = stops()
        assert rc == L.OK and k_stop == [-1] * 3 and status == [0] * 3
        assert lib.prcg_batch_iterate(bt, 60) == L.OK
        rc, k_stop, status = stops()
        assert rc == L.OK and (k_stop[0], status[0]) == (want['k_stop'], CONVERGED) and (k_stop[1:], status[1:]) == ([-1, -1], [0, 0])
        assert lib.prcg_batch_iteration(bt) == 60
        rr = batch.get_scalars(k_stop[0], 0)[4], batch.get_scalars(k_stop[0] - 1, 0)[4]
        assert rr[0] <= thr0 < rr[1]
        assert lib.prcg_batch_get_stops(bt, None, None) == L.EINVAL and 'null buffer' in error()
        # set_stop(NULL): sessions begun from now on launch the plain kernels
        assert lib.prcg_batch_set_stop(bt, None) == L.OK
        rc, k_stop, status = stops()
        assert rc == L.OK and status[0] == CONVERGED, 'the open session is not affected'
        assert lib.prcg_batch_begin(bt, L.HS, L.ptr(rhs), L.ptr(x0), 11, 1) == L.OK
        cleared = record()
        rc, k_stop, status = stops()
        assert rc == L.OK and k_stop == [-1] * 3 and status == [0] * 3
        never = np.zeros(3)
        assert lib.prcg_batch_set_stop(bt, L.ptr(never)) == L.OK
        assert lib.prcg_batch_begin(bt, L.HS, L.ptr(rhs), L.ptr(x0), 11, 1) == L.OK
        with_zero = record()
        rc, k_stop, status = stops()
        assert rc == L.OK and k_stop == [-1] * 3 and status == [0] * 3
    finally:
        batch.close()
    fresh = amd['device'].DeviceBatch([A for A, _ in systems])   # an object that never saw a threshold
    try:
        fresh.begin(L.HS, [b for _, b in systems], [np.zeros(b.size) for _, b in systems], 11, hist_mask=1)
        fresh.iterate(10)
        fresh.sync()
        k_stop, status = fresh.stops()
        assert k_stop.tolist() == [-1] * 3 and status.tolist() == [0] * 3
        plain = ([fresh.get_vector(v, 0) for v in ('x', 'r', 'p', 's')], np.array([fresh.get_scalars(k, 0) for k in range(11)]),
                 np.array([fresh.get_coefficients(k, 0) for k in range(1, 11)]))
    finally:
        fresh.close()
    for got in (cleared, with_zero):
        assert all(np.array_equal(a, b) for a, b in zip(got[0], plain[0])) and np.all(np.isfinite(plain[0][0]))
        assert np.array_equal(got[1], plain[1]) and np.array_equal(got[2], plain[2])
    # the Python object reports the library's text, and clears an earlier session's thresholds
    batch = amd['device'].DeviceBatch([systems[0][0]])
    try:
        batch.begin(L.PIPE_PR, [systems[0][1]], [np.zeros(112)], 11, rr_stop=1e300)
        batch.iterate(10)
        assert [q.tolist() for q in batch.stops()] == [[0], [CONVERGED]]
        batch.begin(L.PIPE_PR, [systems[0][1]], [np.zeros(112)], 11)
        batch.iterate(10)
        assert [q.tolist() for q in batch.stops()] == [[-1], [0]]
    finally:
        batch.close()


@pytest.mark.gpu
def test_the_public_functions(amd, nine, oracle, nine_thr):
    cgv, cbs = amd['cgv'], amd['cbs']
    max_iter = ITERS + 1
    As, bs, x0s = [A for A, _ in nine], [b for _, b in nine], [np.zeros(b.size) for _, b in nine]
    out = cgv.pipe_pr_pcg_batch(As, bs, x0s, max_iter, preconditioner=[cgv.Jacobi(A) for A in As], rtol=RTOL,
                                callbacks=[cbs.updated_residual_2_norm])
    assert len(out) == 9
    for name, thr, trial in zip(NAMES, nine_thr, out):
        want = oracle(name, 'PIPE_PR', thr)
        assert trial['status'] == ('converged' if want['status'] == CONVERGED else 'max_iter'), name
        assert trial['iterations'] == want['last'] and isinstance(trial['iterations'], int), name
        hist = trial['updated_residual_2_norm']
        assert hist.shape == (max_iter,) and np.array_equal(hist[:want['last'] + 1], want['hist']), name
        assert np.array_equal(hist[want['last'] + 1:], np.zeros(ITERS - want['last'])), name
    assert {t['status'] for t in out} == {'converged', 'max_iter'}
    # atol, one value per system, without a preconditioner
    pick = [NAMES.index('nos4'), NAMES.index('lap32x32'), NAMES.index('494_bus')]
    atol = np.array([1e-6 * np.linalg.norm(bs[i]) for i in pick])
    atol[2] = 0.0                                                # never met: this one runs out
    out = cgv.hs_cg_batch([As[i] for i in pick], [bs[i] for i in pick], [x0s[i] for i in pick], max_iter, atol=atol,
                          callbacks=[cbs.updated_residual_2_norm])
    wants = [oracle(NAMES[i], 'HS', a * a, jacobi=False) for i, a in zip(pick, atol)]
    assert [w['status'] for w in wants] == [CONVERGED, CONVERGED, 0], 'the inputs: two converge, one runs out'
    for want, trial in zip(wants, out):
        assert trial['status'] == ('converged' if want['status'] else 'max_iter') and trial['iterations'] == want['last']
        hist = trial['updated_residual_2_norm']
        assert np.array_equal(hist[:want['last'] + 1], want['hist']) and np.array_equal(hist[want['last'] + 1:], np.zeros(ITERS - want['last']))
    # breakdown has a name too
    A, b = indefinite()
    out = cgv.pipe_pr_m_cg_batch(A, [b], [np.zeros(64)], 5, rtol=RTOL)
    assert out[0]['status'] == 'breakdown' and out[0]['iterations'] == 0 and 'updated_residual_2_norm' not in out[0]
    # without rtol / atol: today's dicts
    out = cgv.hs_cg_batch([As[i] for i in pick], [bs[i] for i in pick], [x0s[i] for i in pick], 31, callbacks=[cbs.updated_residual_2_norm])
    plain = run_batch(amd, [nine[i] for i in pick], 'HS', None, chunks=(30,), jacobi=False)
    for s, (trial, rec) in enumerate(zip(out, plain)):
        assert sorted(trial) == ['max_iter', 'name', 'system', 'updated_residual_2_norm'] and trial['system'] == s
        assert np.array_equal(trial['updated_residual_2_norm'], rec['hist'])
