"""ONE DeviceBatch of the nine systems of tests/small_batch_common.py runs every kind of batch session right after every other kind
-- all 18 * 18 ordered pairs, self-pairs included, each exactly once (tests/handle_walk_common.py: 325 runs) -- and every run is
compared, on the 64-bit patterns (NaNs included: a diagonal system that has converged exactly leaves 0 / 0 behind), with the same
kind's run on a batch that has run nothing else.  The fresh batch is the reference; prcg_batch keeps rr_stop, prec, hs, jacobi and
stopping between begins ("may be called again"), and its state, partial and stop-word buffers are reused from session to session.

Kinds: {PIPE_PR, PIPE_PR_M, HS} x {plain, inv_diag, block_jacobi (blocks of 3, a short last block where 3 does not divide n)} x
{no threshold, rr_stop per system}.  Each is held to the oracle under the workgroup's sum on a fresh batch by tests/test_small_batch.py
(plain), test_small_batch_jacobi.py (inv_diag), test_small_batch_block_jacobi.py (block_jacobi) and test_small_batch_stop.py (rr_stop;
with blocks test_small_batch_block_jacobi.py).

Run shape: max_iter = 13, iterate(5); iterate(7), x0 = 0, the recurrence residual recorded.  Compared per system: get_vector of every
name of L.VEC (None where the session does not serve it), scalars of rows 0..12, coefficients of rows 1..12, the history, stops(), k.

Thresholds, from the oracle alone (plan(), asserted without a GPU): system s of a stopping kind takes rr of a row of that kind's own
free oracle run under the workgroup's sum (small_batch_common.wg_dot restates the device's order exactly, as
tests/test_small_batch_stop.py relies on): of the rows 1..11 at which r.r falls below every earlier row -- the only rows a threshold
on r.r can stop a run AT -- the one nearest to 2 + s, so the systems stop at different iterations inside the run; a system whose
r.r never falls below its first value within the run (several of these matrices were chosen because they do that) takes 1e-4 of
rr[0] and runs to the end or to its breakdown.  Where the oracle stops each system under its threshold is what the fresh batch's
stops() must equal.

Two passes: `read` -- every session run to its end and read; `abandoned` -- after the compared run the same kind is begun again,
iterate(3) is called and nothing else, and the next kind begins.

Measured on an MI355X (every pair equal in both passes): 3.4 s (read, with the 18 fresh batches: 0.5 s) and 2.4 s (abandoned)."""
import functools
import itertools

import numpy as np
import pytest

import handle_walk_common as hw
import small_batch_blocks_common as sbb
import small_batch_common as sbc

MAX_ITER = 13
CALLS = (5, 7)
KINDS = [f'{v}-{p}-{"stop" if stop else "free"}' for v, p, stop in itertools.product(sbc.VARIANTS, ('plain', 'jacobi', 'blocks'), (False, True))]
PASSES = ('read', 'abandoned')


def parts(kind):
    variant, prec, stop = kind.split('-')
    return variant, prec, stop == 'stop'


@functools.lru_cache(maxsize=None)
def plan():
    """the nine systems, their block objects, and per stopping kind the thresholds and the oracle's stops: computed once, left unchanged"""
    import new_cg_variants_amd.cg_variants as cgv
    import oracle.ne_oracle as O
    from conftest import _LazyMatrices
    matrices = _LazyMatrices()
    systems = [sbc.system(matrices, name) for name, _, _ in sbc.NINE]
    precs = [cgv.VarBlockJacobi(A, sbb.uniform(A.shape[0], 3)) for A, _ in systems]
    P = dict(systems=systems, blocks=sbb.blocks_of(precs), inv_diag=sbc.jacobi_of(systems), thr={}, stops={})
    iters = MAX_ITER - 1
    for kind in KINDS:
        variant, prec, stop = parts(kind)
        if not stop:
            continue
        thr, stops = [], []
        for s, (A, b) in enumerate(systems):
            M = {'plain': None, 'jacobi': O.jacobi(A), 'blocks': precs[s]}[prec]
            free = sbb.trajectory(A, b, variant, M, thr=0.0, free=0, cap=iters)[1]          # (thr = 0: to the end, or to a breakdown)
            rr = free['scalars'][:, 4]
            last = len(rr) - 2 if free['status'] else len(rr) - 1
            records = [k for k in range(1, min(last, iters - 1) + 1) if np.isfinite(rr[:k + 1]).all() and rr[k] < rr[:k].min()]
            t = float(rr[min(records, key=lambda k: abs(k - (2 + s)))]) if records else 1e-4 * float(rr[0])
            halt = sbb.trajectory(A, b, variant, M, thr=t, free=0, cap=iters)[1]
            thr.append(t)
            stops.append((int(halt['k_stop']), int(halt['status'])))
        P['thr'][kind], P['stops'][kind] = np.array(thr), stops
    return P


def test_the_plan_stops_systems_inside_the_run_at_different_iterations():
    """no GPU: every threshold is a positive finite number; under each stopping kind systems stop converged after their start and
    before the run's last iteration, at differing iterations, beside systems that do not (three and two: the least that makes the
    per-system stop words of one launch differ from each other and from a session without thresholds)"""
    P = plan()
    assert len(KINDS) == 18 and len(hw.all_pairs_sequence(len(KINDS))) == 325 and len(P['thr']) == 9
    for kind, thr in P['thr'].items():
        assert np.isfinite(thr).all() and (thr > 0).all(), (kind, thr)
        inside = [k for k, status in P['stops'][kind] if status == sbc.CONVERGED and 0 < k < MAX_ITER - 1]
        assert len(inside) >= 3 and len(set(inside)) >= 2, (kind, P['stops'][kind])


def begin(kind, L, batch, P):
    variant, prec, stop = parts(kind)
    systems = P['systems']
    batch.begin(getattr(L, variant), [b for _, b in systems], [np.zeros(b.size) for _, b in systems], MAX_ITER, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM,
                inv_diag=P['inv_diag'] if prec == 'jacobi' else None, block_jacobi=P['blocks'] if prec == 'blocks' else None,
                rr_stop=P['thr'][kind] if stop else None)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run(kind, L, batch, P):
    """one session of `kind` on the batch, run to its end and read back in full, floating-point values as their bit patterns"""
    begin(kind, L, batch, P)
    for c in CALLS:
        batch.iterate(c)
    batch.sync()
    k_stop, status = batch.stops()
    out = dict(k=int(batch.k), k_stop=k_stop.copy(), status=status.copy(), systems=[])
    for s in range(len(P['systems'])):
        at = {}
        for v in L.VEC:
            try:
                at[v] = bits(batch.get_vector(v, s))
            except L.PrcgError:
                at[v] = None                   # not part of this session: on both batches or on neither
        out['systems'].append(dict(at=at, scalars=bits(np.array([batch.get_scalars(k, s) for k in range(MAX_ITER)])),
                                   coef=bits(np.array([batch.get_coefficients(k, s) for k in range(1, MAX_ITER)])),
                                   hist=bits(batch.history(s)['updated_residual_2_norm'])))
    return out


def abandon(kind, L, batch, P):
    begin(kind, L, batch, P)
    batch.iterate(3)


def check_fresh(fresh, P):
    """non-vacuity, on the reference runs: the stops are the oracle's, a session without thresholds stops nothing, every session
    serves x, r, p, s, and no two kinds end at the same x in all nine systems"""
    n_sys = len(P['systems'])
    for kind, rec in fresh.items():
        variant, prec, stop = parts(kind)
        assert rec['k'] == MAX_ITER - 1, (kind, rec['k'])
        want = P['stops'][kind] if stop else [(-1, 0)] * n_sys
        assert list(zip(rec['k_stop'].tolist(), rec['status'].tolist())) == want, (kind, rec['k_stop'], rec['status'], want)
        for s, col in enumerate(rec['systems']):
            assert all(col['at'][v] is not None for v in ('x', 'r', 'p', 's')), (kind, s)
            if prec != 'plain' and variant != 'HS':
                assert col['at']['rt'] is not None and col['at']['st'] is not None, (kind, s)
    xs = {kind: np.concatenate([col['at']['x'] for col in rec['systems']]) for kind, rec in fresh.items()}
    same = [(a, b) for a, b in itertools.combinations(fresh, 2) if np.array_equal(xs[a], xs[b])]
    assert not same, ('kinds whose nine systems all end at the same x bit for bit', same)


_fresh = {}


def fresh_runs(L, device, P):
    if not _fresh:
        recs = {}
        for kind in KINDS:
            batch = device.DeviceBatch([A for A, _ in P['systems']])
            try:
                recs[kind] = run(kind, L, batch, P)
            finally:
                batch.close()
        check_fresh(recs, P)
        _fresh.update(recs)
    return _fresh


@pytest.mark.gpu
@pytest.mark.parametrize('how', PASSES)
def test_every_batch_session_after_every_other_equals_a_fresh_batch(how):
    import time
    from new_cg_variants_amd import _lib as L
    from new_cg_variants_amd import device
    P = plan()
    t0 = time.perf_counter()
    fresh = fresh_runs(L, device, P)
    t1 = time.perf_counter()
    batch = device.DeviceBatch([A for A, _ in P['systems']])
    try:
        got = hw.walk(KINDS, lambda kind: run(kind, L, batch, P), fresh, leave=(lambda kind: abandon(kind, L, batch, P)) if how == 'abandoned' else None)
    finally:
        batch.close()
    K = len(KINDS)
    print(f'batch {how}: {got.compared} runs compared, {len(got.found)} differ; fresh batches {t1 - t0:.2f} s, walk {time.perf_counter() - t1:.2f} s')
    assert got.compared == K * K + 1 == 325
    assert len(set(zip(got.sequence, got.sequence[1:]))) == K * K
    assert not got.found, f'pass {how}:\n' + hw.render(KINDS, got.found)
