"""A batch of small systems preconditioned by a diagonal scaling applied inside the one-workgroup solver (prcg.h:
prcg_batch_begin_jacobi; device.DeviceBatch.begin(inv_diag=...); cg_variants.*_pcg_batch).

CPU: the Python argument checks, header and binding, the planner hook under the preconditioned fit rule, and the NumPy model of
the workgroup's sum that the GPU tests hand to the oracle as `dot=`.
GPU: the whole trajectory of the nine systems of test_small_batch.py against oracle/ne_oracle.py, bit for bit; one forced step
of a single Jacobi session from the batch's state; the identity scaling against the unpreconditioned batch; cutting, order and
company; a shared matrix with more systems than CUs and two scalings; isolation of a poisoned scaling; the oracle's golden
histories; the refusals of the C-ABI.

A note on isolation: a NaN in inv_diag reaches r~ = d r, not r = b - A x0, so the poisoned system's row 0 carries NaN in
mu, delta, gamma and nu while rr_0 = r.r -- history entry 0 -- is the clean run's; from entry 1 on the history is NaN.  The test
asserts exactly that (history entry 0 cannot be NaN while row 0 equals the oracle's, which the trajectory test requires)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT, load_run
from small_batch_common import (CONVERGED, FLAVOUR, NINE, VARIANTS, csr_cat, holds_oracle, jacobi_of, oracle_stopped, plan, run_stopping_batch,
                                shape_of, slots, system, thresholds, vectors_of, wg_dot, wg_sum)

ITERS = 60
STOPS = (0, 1, 7, 8, 60)                 # where the vectors are read: 0, 1, 7, 60 against the oracle, 8 for the forced step from 7
CAP = 156 * 1024


def near_cap_matrix():
    """n = 1500 (matrix in LDS), nnz = 9268: 2 * 16 n + 64 * 8 + 12 nnz + 16 = 159744 bytes, the cap exactly -- it fits the
    unpreconditioned solver and misses the preconditioned one by its extra 128 bytes."""
    n, extra = 1500, 268
    lens = np.full(n, 6)
    lens[:extra] += 1
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    indices = np.concatenate([(i + 37 * np.arange(lens[i])) % n for i in range(n)]).astype(np.int32)
    data = np.where(indices == np.repeat(np.arange(n), lens), 10.0, 1.0)
    A = sp.csr_matrix((data, indices, indptr), shape=(n, n))
    assert A.nnz == 9268 and 32 * n + 512 + 12 * A.nnz + 16 == CAP
    return A


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_workgroup_sum_model():
    rng = np.random.default_rng(3)
    for n in (1, 48, 63, 64, 65, 112, 1024, 1025, 1600, 4096):
        v = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
        got = wg_sum(v)
        assert isinstance(got, np.float64)
        assert abs(got - np.sum(v.astype(np.longdouble))) <= 4096 * np.finfo(float).eps * np.sum(np.abs(v))
    # the order, spelled out on a size where every level has something to add: thread t sums rows t, t + 1024, ...; lane l of a
    # wave then adds lane l + 32, l + 16, ..., l + 1; the 16 wave partials are added by halves 8, 4, 2, 1
    v = rng.standard_normal(2500)
    p = np.zeros(4096)
    p[:2500] = v
    thread = [((0.0 + p[t]) + p[t + 1024]) + p[t + 2048] + p[t + 3072] for t in range(1024)]
    level = np.array(thread).reshape(16, 64)
    for off in (32, 16, 8, 4, 2, 1):
        level = np.array([[w[l] + w[l + off] for l in range(off)] for w in level])
    w = level[:, 0]
    for off in (8, 4, 2, 1):
        w = np.array([w[l] + w[l + off] for l in range(off)])
    assert wg_sum(v) == w[0]
    # exact on integers, +0.0 on nothing, nan and inf go through
    assert wg_sum(np.arange(4096.0)) == 4095 * 4096 / 2 and wg_sum(np.zeros(5)) == 0.0
    assert np.isnan(wg_sum(np.array([1.0, np.nan]))) and wg_sum(np.array([1.0, np.inf])) == np.inf
    assert wg_dot(np.array([1.0, 2.0, 3.0]), np.array([4.0, 5.0, 6.0])) == 32.0


def test_planner_hook_under_the_preconditioned_fit_rule(matrices):
    shapes = [shape_of(system(matrices, name)[0]) for name, _, _ in NINE]
    rc, mode, group = plan(shapes)
    rc_j, mode_j, group_j = plan(shapes, jacobi=True)
    assert rc_j == rc == 2 and mode_j.tolist() == mode.tolist() == [m for _, _, m in NINE] and group_j.tolist() == group.tolist()
    # what fits neither
    big = shape_of(matrices['bcsstk14'][0])
    assert plan(shapes + [big], jacobi=True)[0] == plan(shapes + [big])[0] == -(9 + 1)
    # a matrix in LDS at the cap exactly: fits without a preconditioner, not with the extra 128 bytes
    near = shape_of(near_cap_matrix())
    assert near == (1500, 9268, 7)
    rc, mode, _ = plan(shapes[:2] + [near])
    assert rc == 2 and mode.tolist() == [1, 1, 0]
    assert plan(shapes[:2] + [near], jacobi=True)[0] == -(2 + 1)
    assert plan([near] + shapes, jacobi=True)[0] == -(0 + 1)
    # 128 bytes below the cap (16 nonzeros fewer would be 192): the first shape the preconditioned rule takes
    for nnz, fits in ((9268, False), (9258, False), (9257, True)):
        assert 32 * 1500 + 528 + 12 * nnz + 128 <= CAP if fits else 32 * 1500 + 528 + 12 * nnz + 128 > CAP
        assert (plan([(1500, nnz, 7)], jacobi=True)[0] == 1) == fits and plan([(1500, nnz, 7)])[0] == 1
    # the register mode never depends on the LDS need; bad arguments as the unpreconditioned hook
    assert plan([(1024, 8 * 1024, 8)], jacobi=True)[0] == 1
    from new_cg_variants_amd import _lib as L
    assert L.lib().prcg_plan_small_batch_jacobi(0, None, None, None, None, None) == 0


def test_header_and_binding():
    from new_cg_variants_amd import _lib as L
    strip = lambda t: re.sub(r'/\*.*?\*/', '', t, flags=re.S)      # noqa: E731
    text = open(os.path.join(ROOT, 'include', 'prcg.h')).read()
    pub = strip(text)
    tst = strip(open(os.path.join(ROOT, 'include', 'prcg_test.h')).read())
    lib = L.lib()
    assert re.search(r'\bprcg_batch_begin_jacobi\s*\(', pub)
    assert 'prcg_batch_begin_jacobi' in L._SIGNATURES and hasattr(lib, 'prcg_batch_begin_jacobi')
    assert re.search(r'\bprcg_plan_small_batch_jacobi\s*\(', tst) and 'prcg_plan_small_batch_jacobi' not in pub
    assert 'prcg_plan_small_batch_jacobi' in L._SIGNATURES and hasattr(lib, 'prcg_plan_small_batch_jacobi')
    assert L._SIGNATURES['prcg_plan_small_batch_jacobi'] == L._SIGNATURES['prcg_plan_small_batch']
    assert lib.prcg_version() == 1
    section = text[text.index('a BATCH of small independent systems'):text.index('typedef struct prcg_batch')]
    for word in ('prcg_batch_begin_jacobi', 'figure_gen.py:43', 'pipe_pr_cg.py:109-193', 'hs_cg.py:70-131', 'inv_diag', 'PRCG_VEC_RT'):
        assert word in section, word
    assert 'no preconditioner.' not in section.replace('\n * ', ' ')


def test_python_argument_checks_come_before_any_device_call(monkeypatch, matrices):
    import new_cg_variants_amd.callbacks as cbs
    import new_cg_variants_amd.cg_variants as cgv
    from new_cg_variants_amd import problems

    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(cgv, 'DeviceBatch', no_device)
    monkeypatch.setattr(cgv, 'DeviceCSR', no_device)
    monkeypatch.setattr(cgv, '_operator', no_device)
    A, b = system(matrices, 'bcsstk03')
    A2 = problems.laplace_2d(8, 8)
    n, n2 = A.shape[0], A2.shape[0]
    d = 1 / A.diagonal()

    class Blocks:
        def __init__(self, bs):
            self.bs, self.inv_blocks = bs, (d.reshape(-1, 1, 1).copy() if bs == 1 else np.tile(np.eye(2), (n // 2, 1, 1)))

    for name in ('pipe_pr_pcg_batch', 'pipe_pr_m_pcg_batch', 'hs_pcg_batch'):
        f = getattr(cgv, name)
        assert name in cgv.__all__ and f.__name__ == name
        bs, x0s = [b, 2 * b, 3 * b], [np.zeros(n)] * 3
        mixed_bs, mixed_x0s = [b, np.ones(n2)], [np.zeros(n), np.zeros(n2)]
        with pytest.raises(ValueError, match=r'sequence of 3 matrices, one per right-hand side -- got 2'):
            f([A, A], bs, x0s, 5, preconditioner=cgv.Jacobi(A))
        with pytest.raises(ValueError, match=r'x0s must hold 3 vectors, one per system -- got 2'):
            f(A, bs, x0s[:2], 5)
        with pytest.raises(ValueError, match=rf'bs must have shape \(3, {n}\)'):
            f(A, np.ones((3, n + 1)), np.zeros((3, n)), 5)
        with pytest.raises(ValueError, match='callback error_A_norm is not served by a batch'):
            f(A, bs, x0s, 5, preconditioner=cgv.Jacobi(A), callbacks=[cbs.error_A_norm])
        with pytest.raises(ValueError, match='x_true is not served by a batch'):
            f(A, bs, x0s, 5, x_true=np.ones(n))
        # not a diagonal scaling
        for prec in (lambda v: A @ v, lambda v: np.roll(v, 1), Blocks(2), 'jacobi', 3.0):
            with pytest.raises(ValueError, match='a batch applies diagonal preconditioners only'):
                f(A, bs, x0s, 5, preconditioner=prec)
        with pytest.raises(ValueError, match=r'preconditioner\[1\] .*a batch applies diagonal preconditioners only'):
            f(A, bs, x0s, 5, preconditioner=[cgv.Jacobi(A), lambda v: A @ v, None])
        # one object, systems of different sizes; a sequence of the wrong length; a diagonal of the wrong size
        with pytest.raises(ValueError, match=r'one preconditioner object for 2 systems of different sizes \[64, 112\]'):
            f([A, A2], mixed_bs, mixed_x0s, 5, preconditioner=cgv.Jacobi(A))
        with pytest.raises(ValueError, match=r'one object or a sequence of 3, one per system -- got 2'):
            f(A, bs, x0s, 5, preconditioner=[cgv.Jacobi(A)] * 2)
        with pytest.raises(ValueError, match=r'preconditioner\[1\] carries a diagonal of shape \(112,\), the system has size 64'):
            f([A, A2], mixed_bs, mixed_x0s, 5, preconditioner=[cgv.Jacobi(A), cgv.Jacobi(A)])
        # what IS served gets as far as the device
        for prec in (None, cgv.Jacobi(A), lambda v: d * v, Blocks(1), [cgv.Jacobi(A), None, lambda v: d * v], (None, None, None)):
            with pytest.raises(AssertionError, match='the device was reached'):
                f(A, bs, x0s, 5, preconditioner=prec, callbacks=[cbs.updated_residual_2_norm])
        with pytest.raises(AssertionError, match='the device was reached'):
            f([A, A2], mixed_bs, mixed_x0s, 5, preconditioner=[cgv.Jacobi(A), cgv.Jacobi(A2)])
        with pytest.raises(AssertionError, match='the device was reached'):
            f([A, A2], mixed_bs, mixed_x0s, 5)
        with pytest.raises(AssertionError, match='the device was reached'):
            f(A, np.ones((4, n)), np.zeros((4, n)), 5, cgv.Jacobi(A))
    # the diagonals a batch is begun with
    got = cgv._batch_diagonals('f', [cgv.Jacobi(A), None, lambda v: d * v, Blocks(1)], [n] * 4)
    assert [np.array_equal(g, w) for g, w in zip(got, (d, np.ones(n), d, d))] == [True] * 4
    assert all(np.array_equal(g, np.ones(q)) for g, q in zip(cgv._batch_diagonals('f', None, [n, n2]), (n, n2)))
    # the unpreconditioned functions still refuse one
    with pytest.raises(ValueError, match='takes no preconditioner'):
        cgv.hs_cg_batch(A, [b], [np.zeros(n)], 5, preconditioner=cgv.Jacobi(A))


def test_device_batch_checks_inv_diag_like_B(monkeypatch):
    """DeviceBatch.begin shapes inv_diag with batch_vectors, as B and X0: a list of vectors or one 2-D array"""
    from new_cg_variants_amd import device
    sizes = [3, 3]
    with pytest.raises(ValueError, match=r'inv_diag must hold 2 vectors, one per system -- got 1'):
        device.batch_vectors('inv_diag', [np.ones(3)], sizes)
    with pytest.raises(ValueError, match=r'inv_diag\[1\] must have shape \(3,\)'):
        device.batch_vectors('inv_diag', [np.ones(3), np.ones(4)], sizes)
    assert device.batch_vectors('inv_diag', np.arange(6.0).reshape(2, 3), sizes).tolist() == list(range(6))
    import inspect
    assert inspect.signature(device.DeviceBatch.begin).parameters['inv_diag'].default is None


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def amd():
    import new_cg_variants_amd.callbacks as cbs
    import new_cg_variants_amd.cg_variants as cgv
    from new_cg_variants_amd import _lib, device, problems
    return dict(cgv=cgv, cbs=cbs, L=_lib, device=device, problems=problems)


@pytest.fixture(scope='module')
def nine(matrices):
    return [system(matrices, name) for name, _, _ in NINE]


def read_vectors(batch, s, variant):
    return {v: batch.get_vector(v, s) for v in vectors_of(variant)}


def run_batch(amd, systems, variant, inv_diag, chunks=(ITERS,), stops=(), mat_of=None, matrices=None):
    """one DeviceBatch session over `systems` [(A, b)], x0 = 0; inv_diag None: unpreconditioned.  One record per system: the
    vectors at k = 0 and at the end (and at every k of `stops` that a chunk ends on), scalars, coefficients, history."""
    L = amd['L']
    mats = [A for A, _ in systems] if matrices is None else matrices
    batch = amd['device'].DeviceBatch(mats, mat_of)
    names = vectors_of(variant) if inv_diag is not None else ('x', 'r', 'p', 's')
    try:
        batch.begin(getattr(L, variant), [b for _, b in systems], [np.zeros(b.size) for _, b in systems], sum(chunks) + 1, hist_mask=1,
                    inv_diag=inv_diag)
        recs = [{'at': {0: {v: batch.get_vector(v, s) for v in names}}, 'row0': batch.get_scalars(0, s)} for s in range(len(systems))]
        for c in chunks:
            batch.iterate(c)
            if batch.k in stops or batch.k == sum(chunks):
                batch.sync()
                for s, rec in enumerate(recs):
                    rec['at'][batch.k] = {v: batch.get_vector(v, s) for v in names}
        batch.sync()
        assert batch.k == sum(chunks)
        for s, rec in enumerate(recs):
            rec['scalars'] = np.array([batch.get_scalars(k, s) for k in range(sum(chunks) + 1)])
            rec['coef'] = np.array([batch.get_coefficients(k, s) for k in range(1, sum(chunks) + 1)])
            rec['hist'] = batch.history(s)['updated_residual_2_norm']
        return recs
    finally:
        batch.close()


def same(a, b, variant, what='', ks=(0, ITERS), vectors=None):
    idx = slots(variant)
    for k in ks:
        for v in vectors or vectors_of(variant):
            assert np.array_equal(a['at'][k][v], b['at'][k][v], equal_nan=True), (what, k, v)
    assert a['scalars'].shape == b['scalars'].shape and np.array_equal(a['scalars'][:, idx], b['scalars'][:, idx], equal_nan=True), (what, 'scalars')
    assert a['coef'].shape == b['coef'].shape and np.array_equal(a['coef'], b['coef'], equal_nan=True), (what, 'coef')
    assert a['hist'].shape == b['hist'].shape and np.array_equal(a['hist'], b['hist'], equal_nan=True), (what, 'hist')


@pytest.fixture(scope='module')
def base(amd, nine):
    """variant -> the records of the nine systems with d = 1 / diag(A), 60 iterations in ONE call: computed once, never modified"""
    cache = {}

    def get(variant):
        if variant not in cache:
            cache[variant] = run_batch(amd, nine, variant, jacobi_of(nine))
        return cache[variant]
    return get


@pytest.fixture(scope='module')
def stopped(amd, nine):
    """the same run cut at k = 1, 7, 8, where the vectors are read"""
    cache = {}

    def get(variant):
        if variant not in cache:
            cache[variant] = run_batch(amd, nine, variant, jacobi_of(nine), chunks=(1, 6, 1, 52), stops=STOPS)
        return cache[variant]
    return get


def oracle_run(A, b, variant, prec_of=None, iters=ITERS, stops=STOPS):
    """the oracle under the workgroup's sum: vectors at `stops`, scalars {mu, delta, gamma, nu, rr}, coefficients, history"""
    import oracle.ne_oracle as O
    prec = (prec_of or O.jacobi)(A)
    hs = variant == 'HS'
    with np.errstate(all='ignore'):
        st = (O.hs_start if hs else O.pipe_start)(A, b, np.zeros(b.size), prec=prec, dot=wg_dot)
        at, scalars, coef = {}, [], []
        for k in range(iters + 1):
            if k:
                a = st.alpha
                if hs:
                    O.hs_advance(A, st, prec=prec, dot=wg_dot)
                    coef.append([a, st.beta, 0.0])
                else:
                    O.pipe_advance(A, st, flavour=FLAVOUR[variant], prec=prec, dot=wg_dot, square=lambda q: q * q)
                    coef.append([a, st.beta, st.nu_pred])
            assert st.k == k
            scalars.append([st.mu, 0.0 if hs else st.dl, 0.0 if hs else st.gm, st.nu, wg_dot(st.r, st.r)])
            if k in stops:
                at[k] = {v: np.array(getattr(st, v), copy=True) for v in vectors_of(variant)}
        scalars = np.array(scalars)
        return dict(at=at, scalars=scalars, coef=np.array(coef), hist=np.sqrt(scalars[:, 4]))


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_whole_trajectory_against_the_oracle(amd, nine, base, stopped, variant):
    idx = slots(variant)
    ncoef = 2 if variant == 'HS' else 3
    for (name, n, _), (A, b), rec, cut in zip(NINE, nine, base(variant), stopped(variant)):
        want = oracle_run(A, b, variant)
        assert np.all(np.isfinite(want['hist'][:10])) and want['hist'][0] > 0, name      # agreement of NaNs cannot carry the test
        assert rec['scalars'].shape == (ITERS + 1, 8) and rec['hist'].shape == (ITERS + 1,) and rec['at'][0]['x'].shape == (n,)
        assert np.array_equal(rec['row0'][idx], want['scalars'][0, idx], equal_nan=True), (name, 'row 0')
        assert np.array_equal(rec['scalars'][:, idx], want['scalars'][:, idx], equal_nan=True), (name, 'scalars')
        assert np.array_equal(rec['coef'][:, :ncoef], want['coef'][:, :ncoef], equal_nan=True), (name, 'coefficients')
        assert np.array_equal(rec['hist'], want['hist'], equal_nan=True), (name, 'history')
        for k in (0, 1, 7, 60):
            got = (rec if k in (0, ITERS) else cut)['at'][k]
            for v in vectors_of(variant):
                assert np.array_equal(got[v], want['at'][k][v], equal_nan=True), (name, k, v)
        same(cut, rec, variant, name)                            # ... and the run that stopped to be read is the run


def tall_systems():
    """Two systems whose threads hold a THIRD and a FOURTH row (the nine stop at n = 1600: two rows).  Diagonal 2.5 + (i mod 7) / 7,
    -1 between rows i and i + 1, b_i = 1 + 0.25 sin(0.37 i).  (a) n = 2100, tridiagonal throughout: three rows per thread, the
    third in 52 threads; (b) n = 3080, coupled only for 2180 <= i < 3079 (or the matrix would not fit LDS beside the vectors):
    four rows per thread, the fourth in 8 threads.  Both live in LDS, at 143,304 and 157,624 bytes of the 159,744 (+ 128 with
    Jacobi)."""
    out = []
    for n, first in ((2100, 0), (3080, 2180)):
        i = np.arange(n)
        link = ((i >= first) & (i < n - 1)).astype(float)[:-1]
        A = sp.csr_matrix(sp.diags([-link, 2.5 + (i % 7) / 7, -link], [-1, 0, 1]))
        A.eliminate_zeros()
        A.sort_indices()
        out.append((A, 1 + 0.25 * np.sin(0.37 * i)))
    assert [shape_of(A)[:2] for A, _ in out] == [(2100, 6298), (3080, 4878)]
    assert [32 * A.shape[0] + 512 + 12 * A.nnz + 16 for A, _ in out] == [143304, 157624] and 157624 + 128 <= CAP
    return out


@pytest.mark.gpu
def test_third_and_fourth_row_of_a_thread(amd):
    """12 iterations of the three variants on tall_systems(), one batch: the Jacobi session against the oracle as in
    test_whole_trajectory_against_the_oracle; d = ones against the unpreconditioned session; and a session stopped at
    (1e-3 ||b||)^2 -- strictly inside the run -- against the stopping oracle, as test_small_batch_stop.py holds the nine."""
    iters, at = 12, (0, 1, 12)
    systems = tall_systems()
    rc, mode, _ = plan([shape_of(A) for A, _ in systems], jacobi=True)
    assert rc == 1 and mode.tolist() == [0, 0]
    thr = thresholds([b for _, b in systems], rtol=1e-3)
    for variant in VARIANTS:
        idx, ncoef = slots(variant), 2 if variant == 'HS' else 3
        # the inputs: finite histories, and a stop strictly inside the run
        wants = [oracle_run(A, b, variant, iters=iters, stops=at) for A, b in systems]
        halts = [oracle_stopped(A, b, variant, t, iters) for (A, b), t in zip(systems, thr)]
        for want, halt in zip(wants, halts):
            assert np.all(np.isfinite(want['hist'])) and want['hist'][0] > 0, variant
            assert halt['status'] == CONVERGED and 1 < halt['k_stop'] < iters, (variant, halt['k_stop'])
        recs = run_batch(amd, systems, variant, jacobi_of(systems), chunks=(1, iters - 1), stops=at)
        for s, (rec, want) in enumerate(zip(recs, wants)):
            assert rec['scalars'].shape == (iters + 1, 8) and rec['hist'].shape == (iters + 1,)
            assert np.array_equal(rec['row0'][idx], want['scalars'][0, idx]), (variant, s, 'row 0')
            assert np.array_equal(rec['scalars'][:, idx], want['scalars'][:, idx]), (variant, s, 'scalars')
            assert np.array_equal(rec['coef'][:, :ncoef], want['coef'][:, :ncoef]), (variant, s, 'coefficients')
            assert np.array_equal(rec['hist'], want['hist']), (variant, s, 'history')
            for k in at:
                for v in vectors_of(variant):
                    assert np.array_equal(rec['at'][k][v], want['at'][k][v]), (variant, s, k, v)
        ones = run_batch(amd, systems, variant, [np.ones(b.size) for _, b in systems], chunks=(iters,))
        plain = run_batch(amd, systems, variant, None, chunks=(iters,))
        for s, (a, b) in enumerate(zip(ones, plain)):
            same(a, b, variant, (variant, s), ks=(0, iters), vectors=('x', 'r', 'p', 's'))
            assert np.array_equal(a['scalars'][:, :5], b['scalars'][:, :5]), (variant, s)
            assert np.all(np.isfinite(b['hist'])) and b['hist'][iters] > 0
        for s, (rec, halt) in enumerate(zip(run_stopping_batch(amd, systems, variant, thr, chunks=(iters,)), halts)):
            holds_oracle(rec, halt, variant, iters, (variant, s))


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['PIPE_PR', 'HS'])
@pytest.mark.parametrize('name', ['bcsstk03', '494_bus'])
def test_one_forced_step_of_a_single_session(amd, nine, stopped, variant, name):
    """A single Jacobi session set to the batch's state at k = 0 and k = 7 -- every vector it holds, w = A r~ and u = A s~ as
    SciPy products -- steps to the batch's vectors at k + 1, bit for bit: pipelined all six; Hestenes-Stiefel x and r, and p and
    s given the single session's own b (see below).  Inner products are not compared: the trees differ."""
    L = amd['L']
    i = [q[0] for q in NINE].index(name)
    (A, b), rec = nine[i], stopped(variant)[i]
    d = 1 / A.diagonal()
    op = amd['device'].DeviceCSR(A)
    try:
        op.begin(getattr(L, variant), b, np.zeros(b.size), ITERS + 1, inv_diag=d)
        for k in (0, 7):
            state = dict(rec['at'][k])
            if variant == 'HS':
                state['rt'] = d * state['r']
            else:
                state['w'], state['u'] = A @ state['rt'], A @ state['st']
                state['wt'], state['ut'] = d * state['w'], d * state['u']
            held = []
            for v, a in state.items():
                try:
                    op.set_vector(v, a)
                    held.append(v)
                except L.PrcgError:
                    pass                                         # not part of this session's device state
            assert set(vectors_of(variant)) <= set(held), held
            op.set_scalars(k, rec['scalars'][k])
            op.set_iteration(k)
            op.iterate(1)
            op.sync()
            if variant != 'HS':                                  # a, b and nu_pred all come from row k: nothing depends on a tree
                for v in vectors_of(variant):
                    assert np.array_equal(op.get_vector(v), rec['at'][k + 1][v]), (name, variant, k, v)
                continue
            # Hestenes-Stiefel: x and r use a = nu_k / mu_k only.  b = nu' / nu_k is formed from nu' = r.r~ summed INSIDE the
            # step, in the single session's tree, so p = r~ + b p and s = A p carry the single session's b (measured: 494_bus
            # differs from the batch's in the last bit, bcsstk03 does not): they are held to the same expressions with that b
            for v in ('x', 'r'):
                assert np.array_equal(op.get_vector(v), rec['at'][k + 1][v]), (name, variant, k, v)
            bt, bt_batch = op.get_coefficients(k + 1)[1], rec['coef'][k][1]
            # two orders of one sum of n nonnegative terms d_i r_i^2: each within (n - 1) u of the exact value, u = eps / 2
            assert abs(bt - bt_batch) <= 2 * A.shape[0] * np.finfo(float).eps * abs(bt_batch), (name, k, bt, bt_batch)
            p1 = d * rec['at'][k + 1]['r'] + bt * rec['at'][k]['p']
            assert np.array_equal(op.get_vector('p'), p1), (name, variant, k, 'p')
            assert np.array_equal(op.get_vector('s'), A @ p1), (name, variant, k, 's')
            if bt == bt_batch:
                assert np.array_equal(p1, rec['at'][k + 1]['p']) and np.array_equal(A @ p1, rec['at'][k + 1]['s']), (name, k)
    finally:
        op.close()


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_the_identity_scaling_is_the_unpreconditioned_batch(amd, nine, variant):
    ones = run_batch(amd, nine, variant, [np.ones(b.size) for _, b in nine])
    plain = run_batch(amd, nine, variant, None)
    for (name, _, _), a, b in zip(NINE, ones, plain):
        same(a, b, variant, name, vectors=('x', 'r', 'p', 's'))
        assert np.array_equal(a['scalars'][:, :5], b['scalars'][:, :5], equal_nan=True), name
        if variant != 'HS':                                      # r~ = r and s~ = s, value for value
            for k in (0, ITERS):
                assert np.array_equal(a['at'][k]['rt'], a['at'][k]['r'], equal_nan=True), name
                assert np.array_equal(a['at'][k]['st'], a['at'][k]['s'], equal_nan=True), name


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_cutting_order_and_company_change_nothing(amd, nine, base, variant):
    want = base(variant)
    d = jacobi_of(nine)
    cut = run_batch(amd, nine, variant, d, chunks=(20, 1, 39))
    for (name, _, _), a, b in zip(NINE, cut, want):
        same(a, b, variant, 'cut ' + name)
    rev = run_batch(amd, nine[::-1], variant, d[::-1])[::-1]
    for (name, _, _), a, b in zip(NINE, rev, want):
        same(a, b, variant, 'reversed ' + name)
    for mode in (1, 0):
        members = [i for i, (_, _, m) in enumerate(NINE) if m == mode]
        part = run_batch(amd, [nine[i] for i in members], variant, [d[i] for i in members])
        for i, a in zip(members, part):
            same(a, want[i], variant, f'mode {mode} alone: ' + NINE[i][0])


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['PIPE_PR', 'HS'])
def test_shared_matrix_two_scalings_and_more_systems_than_cus(amd, matrices, variant):
    L = amd['L']
    A, b = system(matrices, 'bcsstk03')
    n, n_sys, iters = A.shape[0], 300, 50
    B = np.array([b * (1 + s % 7) for s in range(n_sys)])
    D = np.array([1 / A.diagonal() if s % 2 == 0 else np.ones(n) for s in range(n_sys)])
    batch = amd['device'].DeviceBatch([A], np.zeros(n_sys, dtype=np.int32))
    try:
        batch.begin(getattr(L, variant), B, np.zeros((n_sys, n)), iters + 1, hist_mask=1, inv_diag=D)
        batch.iterate(iters)
        batch.sync()
        X = batch.solutions()
        assert X.shape == (n_sys * n,)
        xs = np.array([batch.get_vector('x', s) for s in range(n_sys)])
        assert np.array_equal(X, xs.reshape(-1), equal_nan=True)
        hists = np.array([batch.history(s)['updated_residual_2_norm'] for s in range(n_sys)])
    finally:
        batch.close()
    assert np.all(np.isfinite(hists[:, :10])) and np.all(np.isfinite(xs[:14]))
    for c in range(14):                                          # equal inputs: equal right-hand side (s mod 7) and scaling (s mod 2)
        assert np.array_equal(xs[c::14], np.broadcast_to(xs[c], xs[c::14].shape), equal_nan=True), c
        assert np.array_equal(hists[c::14], np.broadcast_to(hists[c], hists[c::14].shape), equal_nan=True), c
    assert not np.array_equal(xs[0], xs[1])
    assert not np.array_equal(xs[0], xs[7]) and not np.array_equal(hists[0], hists[7])      # one right-hand side, two scalings


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_a_poisoned_scaling_stays_in_its_system(amd, nine, base, variant):
    want = base(variant)
    for poison in (np.nan, 0.0):
        d = jacobi_of(nine)
        d[3][5] = poison
        got = run_batch(amd, nine, variant, d)
        for i, ((name, _, _), a, b) in enumerate(zip(NINE, got, want)):
            if i != 3:
                same(a, b, variant, f'{poison}: {name}')
        if np.isnan(poison):
            # r~ = d r is NaN from the start: mu and nu of row 0 (and delta, gamma) are NaN; rr_0 = r.r does not see d, so
            # history entry 0 is the clean run's and every later entry is NaN
            row0 = got[3]['scalars'][0]
            assert np.all(np.isnan(row0[[0, 3]])) and (variant == 'HS' or np.all(np.isnan(row0[[1, 2]])))
            assert got[3]['hist'][0] == want[3]['hist'][0] and np.all(np.isnan(got[3]['hist'][1:]))
            assert np.all(np.isnan(got[3]['at'][ITERS]['x']))
        # (a zero entry makes the scaling singular: inf and nan are allowed in system 3, nowhere else)


@pytest.mark.gpu
@pytest.mark.parametrize('fn,method', [('pipe_pr_pcg_batch', 'pipe_pr_pcg'), ('hs_pcg_batch', 'hs_pcg')])
def test_against_the_oracles_golden_histories(amd, matrices, fn, method):
    from test_gpu_parity import PREFIX_FLOOR
    cgv, cbs = amd['cgv'], amd['cbs']
    names = ['bcsstk03', 'nos7']
    systems = [system(matrices, name) for name in names]
    max_iter = 40
    As, bs, x0s = [A for A, _ in systems], [b for _, b in systems], [np.zeros(b.size) for _, b in systems]
    out = getattr(cgv, fn)(As, bs, x0s, max_iter, preconditioner=[cgv.Jacobi(A) for A in As], callbacks=[cbs.updated_residual_2_norm])
    assert len(out) == 2
    for name, trial in zip(names, out):
        ref = load_run(name, method, 'jacobi')['hist_updated_residual_2_norm']
        prefix = PREFIX_FLOOR[name]
        assert trial['name'] == fn and trial['max_iter'] == max_iter and trial['updated_residual_2_norm'].shape == (max_iter,)
        print(name, fn, 'jacobi', np.abs(trial['updated_residual_2_norm'][:prefix] / ref[:prefix] - 1).max())
        np.testing.assert_allclose(trial['updated_residual_2_norm'][:prefix], ref[:prefix], rtol=1e-12, atol=0, err_msg=f'{name}/{fn}')
    # no preconditioner: the identity, as the reference's *_pcg called without one
    out = getattr(cgv, fn)(As[0], bs[:1], x0s[:1], max_iter, preconditioner=None, callbacks=[cbs.updated_residual_2_norm])
    ref = load_run('bcsstk03', method, 'None')['hist_updated_residual_2_norm']
    prefix = PREFIX_FLOOR['bcsstk03']
    print('bcsstk03', fn, 'None', np.abs(out[0]['updated_residual_2_norm'][:prefix] / ref[:prefix] - 1).max())
    np.testing.assert_allclose(out[0]['updated_residual_2_norm'][:prefix], ref[:prefix], rtol=1e-12, atol=0, err_msg=f'bcsstk03/{fn}/None')


@pytest.mark.gpu
def test_refusals_through_the_c_abi(amd, matrices):
    L = amd['L']
    lib = L.lib()
    A3, b3 = system(matrices, 'bcsstk03')
    A4 = system(matrices, 'nos4')[0]
    near = near_cap_matrix()
    op = amd['device'].DeviceCSR(A3)                 # an ordinary handle with an operator: left alone by every refusal
    h = op._h

    def create(mats, mat_of):
        rows_off, nnz_off, indptr, indices, data = csr_cat(mats)
        mat_of = np.asarray(mat_of, dtype=np.int32)
        out = C.c_void_p()
        rc = lib.prcg_batch_create(h, len(mats), L.ptr(rows_off), L.ptr(nnz_off), L.ptr(indptr), L.ptr(indices), L.ptr(data), len(mat_of),
                                   L.ptr(mat_of), C.byref(out))
        assert rc == L.OK and out.value, lib.prcg_last_error(h)
        return out

    def error():
        return (lib.prcg_last_error(h) or b'').decode()

    def get(bt, which, s, n):
        out = np.full(n, -1.0)
        return lib.prcg_batch_get_vector(bt, which, s, L.ptr(out)), out
    n3, n4 = A3.shape[0], A4.shape[0]
    try:
        # ---- a batch whose system 3 lies at the LDS cap: every reason, each decided before a device call
        bt = create([A3, A4, near], [0, 1, 0, 2])
        try:
            n_all = 2 * n3 + n4 + near.shape[0]
            rhs, x0, dinv = np.ones(n_all), np.zeros(n_all), np.ones(n_all)

            def begin_refused(text, variant=L.PIPE_PR, r=rhs, x=x0, d=dinv, max_iter=5, mask=1):
                rc = lib.prcg_batch_begin_jacobi(bt, variant, L.ptr(r), L.ptr(x), L.ptr(d), max_iter, mask)
                assert rc == L.EINVAL and re.search(text, error()), (rc, error())
            # an open unpreconditioned session, which every refusal must leave alone
            assert lib.prcg_batch_begin(bt, L.HS, L.ptr(rhs), L.ptr(x0), 5, 1) == L.OK and lib.prcg_batch_iterate(bt, 2) == L.OK
            for variant in (L.PIPE_P, L.PIPE_P_M, L.PR, L.M, L.CG_CG, L.GV, 99, -1):
                begin_refused(rf'prcg_batch_begin_jacobi: variant {variant} is not served by a batch', variant=variant)
            for mask in (2, 4, 8, 3, 16):
                begin_refused(rf'history bits {mask}', mask=mask)
            begin_refused(r'null rhs, x0 or inv_diag', r=None)
            begin_refused(r'null rhs, x0 or inv_diag', x=None)
            begin_refused(r'null rhs, x0 or inv_diag', d=None)
            begin_refused(r'max_iter = 0', max_iter=0)
            begin_refused(r'max_iter = -3', max_iter=-3)
            for variant in (L.PIPE_PR, L.PIPE_PR_M, L.HS):
                begin_refused(r'system 3 \(n = 1500, nnz = 9268\) fits the one-workgroup solver without a preconditioner but not with one',
                              variant=variant)
            # ... nothing was changed: the session goes on, and the same object begins another
            assert lib.prcg_batch_iteration(bt) == 2 and lib.prcg_batch_iterate(bt, 2) == L.OK and lib.prcg_batch_sync(bt) == L.OK
            assert lib.prcg_batch_iteration(bt) == 4
            assert lib.prcg_batch_begin(bt, L.PIPE_PR, L.ptr(rhs), L.ptr(x0), 5, 1) == L.OK
            assert lib.prcg_batch_iterate(bt, 4) == L.OK and lib.prcg_batch_sync(bt) == L.OK and lib.prcg_batch_iteration(bt) == 4
            hist = np.zeros(5)
            assert lib.prcg_batch_get_history(bt, 3, L.ptr(hist)) == L.OK and np.all(np.isfinite(hist)) and hist[0] > 0
        finally:
            lib.prcg_batch_destroy(bt)
        # ---- r~ and s~ belong to a pipelined Jacobi session only
        bt = create([A3, A4], [0, 1, 0])
        try:
            n_all = 2 * n3 + n4
            rhs, x0, dinv = np.ones(n_all), np.zeros(n_all), np.full(n_all, 0.5)
            assert lib.prcg_batch_begin(bt, L.PIPE_PR, L.ptr(rhs), L.ptr(x0), 5, 1) == L.OK
            for which in (L.VEC['rt'], L.VEC['st']):
                rc, out = get(bt, which, 1, n4)
                assert rc == L.EINVAL and re.search(r'this session is unpreconditioned', error()) and np.all(out == -1.0)
            assert lib.prcg_batch_begin_jacobi(bt, L.HS, L.ptr(rhs), L.ptr(x0), L.ptr(dinv), 5, 1) == L.OK
            for which in (L.VEC['rt'], L.VEC['st']):
                rc, out = get(bt, which, 1, n4)
                assert rc == L.EINVAL and re.search(r'this session is Hestenes-Stiefel', error()) and np.all(out == -1.0)
            for which in (L.VEC['w'], L.VEC['u'], L.VEC['wt'], L.VEC['ut'], 17):
                rc, out = get(bt, which, 1, n4)
                assert rc == L.EINVAL and re.search(rf'vector {which} is not part of a batch session', error())
            assert lib.prcg_batch_begin_jacobi(bt, L.PIPE_PR_M, L.ptr(rhs), L.ptr(x0), L.ptr(dinv), 5, 1) == L.OK
            rc, r = get(bt, L.VEC['r'], 1, n4)
            rc2, rt = get(bt, L.VEC['rt'], 1, n4)
            assert rc == rc2 == L.OK and np.array_equal(r, np.ones(n4)) and np.array_equal(rt, 0.5 * r)
            rc, s = get(bt, L.VEC['s'], 1, n4)
            rc2, st = get(bt, L.VEC['st'], 1, n4)
            assert rc == rc2 == L.OK and np.array_equal(s, A4 @ rt) and np.array_equal(st, 0.5 * s)
            # ... and the same object still runs a prcg_batch_begin session
            assert lib.prcg_batch_begin(bt, L.HS, L.ptr(rhs), L.ptr(x0), 5, 1) == L.OK
            assert lib.prcg_batch_iterate(bt, 4) == L.OK and lib.prcg_batch_sync(bt) == L.OK and lib.prcg_batch_iteration(bt) == 4
        finally:
            lib.prcg_batch_destroy(bt)
        # after all the refusals the handle still serves an ordinary single session
        op.begin(L.PIPE_PR, b3, np.zeros(b3.size), 21, hist_mask=1)
        op.iterate(20)
        ref = load_run('bcsstk03', 'pipe_pr_cg', 'None')['hist_updated_residual_2_norm']
        np.testing.assert_allclose(op.history()['updated_residual_2_norm'][:7], ref[:7], rtol=1e-12)
    finally:
        op.close()
    # the Python object reports the library's text
    batch = amd['device'].DeviceBatch([A3, near])
    try:
        with pytest.raises(L.PrcgError, match=r'system 1 \(n = 1500, nnz = 9268\)'):
            batch.begin(L.PIPE_PR, [b3, np.ones(1500)], [np.zeros(n3), np.zeros(1500)], 5, inv_diag=[np.ones(n3), np.ones(1500)])
    finally:
        batch.close()
