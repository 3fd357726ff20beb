"""The four kinds of session that stop on the device -- pipelined single (prcg_set_stop), per-column two-RHS (prcg_set_stop_rhs),
Hestenes-Stiefel (prcg_set_stop_hs) and block-Jacobi pipelined (prcg_set_stop_block_jacobi) -- share ONE word buffer on the handle,
one block of session state and one routine that prcg_sync resolves a stop with.  Each kind is held to the oracle on a handle of
its own by test_single_stop.py, test_multi_rhs_stop.py, test_hs_stop.py and test_block_jacobi_stop.py; this module runs them BACK
TO BACK on one handle, with sessions without a threshold between them, forwards and then in the reverse order, and compares every
session with the same session on a freshly opened handle, for equal bits.  The fresh runs are the reference.

Two operators: s1_small (window tiles: a one-launch pipelined session flips its input pairs, a Hestenes-Stiefel session its two
direction buffers) and fem_like_3d(12) (sliced rows: the four-vector product, in-place directions).  Run lengths are those of the
tables of the four modules for these operators (10 and 32; the two-RHS reference runs of fem12: 60); s1_small has no two-RHS or
block-Jacobi entry there and takes its own 10.

Thresholds, all from the oracle on the CPU (plan, asserted by test_the_plan_stops_every_session_inside_its_run):
 * two-RHS and block-Jacobi sessions run two-kernel schedules whose every sum device_order.device_dot restates exactly: thr = rr of
   an oracle row, as in their own modules -- rows (20, 45) of the fem12 table, (3, 7) of ten for s1_small; block Jacobi: rr of
   row max_iter // 2;
 * the one-launch pipelined and the Hestenes-Stiefel sessions sum in an order that depends on the launch (a tree the session
   reports), which the CPU does not know here: thr = the geometric mean of rr at k and k - 1, k the first row with rr <= rr at
   max_iter // 2 under device_dot / np.dot.  The plan asserts that every earlier rr lies above thr and rr_k below it by more than
   one part in 1000 -- two summation orders differ by some n * 2^-53 ~ 1e-12 per inner product, which 32 iterations of these
   well-conditioned runs do not amplify by nine orders of magnitude -- so the device stops at that k whatever its tree.
Each stopping single session is iterated k_stop + 1 times and synchronised: the stop lies ONE launch before the end of the call, an
odd distance, so resolving it must take a buffer flip back; the rest of the run then finds the session stopped."""
import functools

import numpy as np
import pytest

import block_jacobi_stop_common as bjc
import hs_stop_common as hsc
import multi_rhs_common as common
import multi_rhs_stop_common as rhsc
import single_stop_common as ssc
from device_order import device_dot

KNOBS = {'PRCG_SMALL': '0'}
# operator -> (max_iter of the single sessions, iterations of the two-RHS sessions, the oracle rows its two thresholds are rr of)
RUNS = {'s1_small': (10, 10, (3, 7)), 'fem12': (32, rhsc.ITERS, (20, 45))}
MARGIN = 1e-3
ORDER = ('pipe_pr', 'rhs2', 'hs', 'block_jacobi', 'pipe_pr_m_free', 'rhs2_free')
BJ_BEGIN = {'block_jacobi': (2, None)}


def between_rows(rr, row):
    """(thr, k): k the first row with rr <= rr[row], thr the geometric mean of rr[k - 1] and rr[k]; and the margins asserted"""
    k = int(np.argmax(rr <= rr[row]))
    thr = float(np.sqrt(rr[k - 1] * rr[k]))
    assert k >= 1 and (rr[:k] > thr * (1 + MARGIN)).all() and rr[k] < thr * (1 - MARGIN), (k, thr, rr[:k + 1])
    return thr, k


@functools.lru_cache(maxsize=None)
def plan(name):
    """Everything the sessions of one operator need, from the CPU alone, computed once and left unchanged: the system, the
    thresholds, and where the oracle stops each session under them"""
    import new_cg_variants_amd.cg_variants as cgv
    A, B, X0 = common.problem(name, 2)
    b = B[0]
    max_iter, iters2, rows = RUNS[name]
    p = dict(A=A, B=B, X0=X0, b=b, max_iter=max_iter, iters2=iters2)
    with np.errstate(all='ignore'):
        traj = ssc.trajectory(A, b, 'pipe_pr_cg', device_dot, device_dot, max_iter - 1, keep=())
        p['pipe_thr'], p['pipe_k'] = between_rows(traj['scalars'][:, 4], max_iter // 2)
        assert ssc.stop_of(traj, p['pipe_thr']) == (p['pipe_k'], ssc.CONVERGED)
        traj = hsc.trajectory_np(A, b, 'hs_cg', max_iter - 1, keep=())
        p['hs_thr'], p['hs_k'] = between_rows(traj['scalars'][:, 4], max_iter // 2)
        assert hsc.stop_of(traj, p['hs_thr']) == (p['hs_k'], hsc.CONVERGED)
        M = cgv.DeviceBlockJacobi(A, 2)
        traj = bjc.trajectory(A, b, 'PIPE_P', M, max_iter - 1)
        p['bj_thr'] = float(traj['scalars'][max_iter // 2, 4])
        p['bj_stop'] = ssc.stop_of(traj, p['bj_thr'])
        rr = [rhsc.reference(name, 'pr', False, c, iters2)['scalars'] for c in range(2)]
        p['rhs_thr'] = [float(rr[c][rows[c], 4]) for c in range(2)]
        p['rhs_stops'] = [rhsc.stop_of(rr[c], p['rhs_thr'][c]) for c in range(2)]
        p['free_finite'] = bool(np.isfinite(ssc.trajectory(A, b, 'pipe_pr_m_cg', device_dot, device_dot, max_iter - 1, keep=())['scalars']).all()
                                and np.isfinite(rr[0]).all() and np.isfinite(rr[1]).all())
    return p


@pytest.mark.parametrize('name', list(RUNS))
def test_the_plan_stops_every_session_inside_its_run(name):
    """no GPU: every stopping session stops strictly inside its run, converged, the two columns at different iterations; the
    sessions without a threshold stay finite to their end (between_rows asserts the margins of the two order-dependent kinds)"""
    p = plan(name)
    m = p['max_iter']
    for k in (p['pipe_k'], p['hs_k']):
        assert 0 < k and k + 1 < m - 1, (name, k)               # the call of k + 1 iterations ends inside the run
    assert p['pipe_thr'] > 0 and p['hs_thr'] > 0
    k, status = p['bj_stop']
    assert status == ssc.CONVERGED and 0 < k < m - 1 and p['bj_thr'] > 0, (name, p['bj_stop'])
    (k0, s0), (k1, s1) = p['rhs_stops']
    assert s0 == s1 == ssc.CONVERGED and 0 < k0 < k1 < p['iters2'] - 1, (name, p['rhs_stops'])
    assert p['free_finite']


def run(kind, L, op, p):
    """one session of `kind` on op, begun, run to its end and read back in full with the reader of that kind's own module"""
    m, it2 = p['max_iter'], p['iters2']
    if kind == 'pipe_pr':
        k = p['pipe_k']
        return ssc.run_session(L, op, 'pipe_pr_cg', p['b'], None, m, p['pipe_thr'], (k + 1,), then=m - 2 - k)
    if kind == 'hs':
        k = p['hs_k']
        return hsc.run_session(L, op, 'hs_cg', p['b'], None, m, p['hs_thr'], (k + 1,), then=m - 2 - k)
    if kind == 'block_jacobi':
        return bjc.run_session(L, op, 'PIPE_P', p['b'], m, p['bj_thr'], (1, 2), BJ_BEGIN, then=3)
    if kind == 'pipe_pr_m_free':
        return ssc.run_session(L, op, 'pipe_pr_m_cg', p['b'], None, m, None, (3, m - 4))
    later = max(k for k, _ in p['rhs_stops'])
    calls = (later + 1, it2 - later - 1) if kind == 'rhs2' else (7, it2 - 7)
    cols, stops, k = rhsc.session(op, L, L.PIPE_PR, p['B'], p['X0'], it2, None, p['rhs_thr'] if kind == 'rhs2' else None, calls)
    return dict(cols=cols, stops=stops, k=k, schedule=op.schedule())


def differences(a, b, path=''):
    """the paths at which two readings differ (np.array_equal at the leaves)"""
    if isinstance(a, dict):
        return [f'{path}: keys'] if a.keys() != b.keys() else [d for key in a for d in differences(a[key], b[key], f'{path}/{key}')]
    if isinstance(a, (list, tuple)) and not np.isscalar(a):
        return [f'{path}: length'] if len(a) != len(b) else [d for i, (x, y) in enumerate(zip(a, b)) for d in differences(x, y, f'{path}[{i}]')]
    if a is None or b is None:
        return [] if a is b else [path]
    return [] if np.array_equal(np.asarray(a), np.asarray(b)) else [path]


def check_stops(kind, rec, p):
    """where the plan says (the fresh run is held to this too, so a plan the device does not follow fails here, not in the comparison)"""
    m, it2 = p['max_iter'], p['iters2']
    if kind in ('pipe_pr', 'hs'):
        k = p['pipe_k' if kind == 'pipe_pr' else 'hs_k']
        assert rec['stop'] == (k, ssc.CONVERGED) and rec['k'] == k, (kind, rec['stop'], rec['k'], k)
        assert rec['again']['stop'] == rec['stop'] and rec['again']['k'] == k
    elif kind == 'block_jacobi':
        assert rec['stop'] == p['bj_stop'] and rec['k'] == p['bj_stop'][0], (kind, rec['stop'], rec['k'])
    elif kind == 'pipe_pr_m_free':
        assert rec['stop'] == (-1, 0) and rec['k'] == m - 1, (kind, rec['stop'], rec['k'])
    elif kind == 'rhs2':
        assert rec['stops'] == p['rhs_stops'] and rec['k'] == max(k for k, _ in p['rhs_stops']), (kind, rec['stops'], rec['k'])
    else:
        assert rec['stops'] == [(-1, 0), (-1, 0)] and rec['k'] == it2, (kind, rec['stops'], rec['k'])


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(RUNS))
def test_sessions_of_every_kind_back_to_back_equal_fresh_handles(name):
    from new_cg_variants_amd import _lib as L
    from new_cg_variants_amd import device
    p = plan(name)
    fresh = {}
    for kind in ORDER:
        op = device.DeviceCSR(p['A'], knobs=dict(KNOBS))
        try:
            fresh[kind] = run(kind, L, op, p)
        finally:
            op.close()
        check_stops(kind, fresh[kind], p)
    assert fresh['pipe_pr']['schedule']['fused'] and fresh['hs']['schedule']['fused'] and fresh['block_jacobi']['schedule']['block_jacobi']
    assert fresh['pipe_pr']['schedule']['window'] == (name == 's1_small') and fresh['rhs2']['schedule']['spmm4'] == (name == 'fem12')
    op = device.DeviceCSR(p['A'], knobs=dict(KNOBS))
    try:
        for kind in ORDER + ORDER[::-1]:
            rec = run(kind, L, op, p)
            check_stops(kind, rec, p)
            diff = differences(rec, fresh[kind])
            assert not diff, (name, kind, 'differs from the same session on a fresh handle at', diff[:8])
    finally:
        op.close()
