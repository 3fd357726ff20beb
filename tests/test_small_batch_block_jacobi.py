"""A batch of small systems preconditioned by point-block Jacobi applied inside the one-workgroup solver (prcg.h:
prcg_batch_begin_block_jacobi; device.DeviceBatch.begin(block_jacobi=...); cg_variants.*_bpcg_batch).

CPU: header and binding, the planner hook under this call's fit rule, the Python argument checks.
GPU: ONE batch of ten systems -- five matrices, uniform and cyclic partitions, systems on one matrix with different partitions
-- held to oracle/ne_oracle.py under the workgroup's sum with VarBlockJacobi.__call__ as `prec=`, bit for bit: 60 free
iterations, and the run stopped at rtol = 1e-8; a partition of ones against prcg_batch_begin_jacobi; blocks that straddle the
rows 1023/1024, 2047/2048 and 3071/3072 of a thread; cutting, order, company, more systems than CUs and a poisoned block; the
refusals of the C-ABI; the Python functions.

The oracle's stops under the workgroup's sum (computed on the CPU, b as small_batch_common.system gives it), rtol = 1e-8:
    system, partition      PIPE_PR        PIPE_PR_M      HS
    bcsstk03  bs 3         173            176            163
    bcsstk03  bs 8          67             67             67
    bcsstk03  cyclic       152            152            141
    nos4      bs 3          74             74             74
    nos7      bs 3          90             90             90
    nos7      bs 8          96 breakdown  111 breakdown   88
    lap32x32  bs 3          62             62             62
    lap32x32  bs 8          56             56             56
    494_bus   cyclic       241            241            241
    494_bus   bs 8         288            288            288
Hestenes-Stiefel does not break down on nos7 with bs 8: the breakdown is asserted for the two pipelined variants."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from small_batch_blocks_common import (FREE, MAX_ITER, NOS7_BS8, RTOL, TEN, blocks_of, cyclic, run_blocks, same_record, tall_system,
                                       ten_systems, trajectory, uniform)
from small_batch_common import BREAKDOWN, CONVERGED, NINE, VARIANTS, csr_cat, holds_oracle, jacobi_of, shape_of, slots, system, thresholds

CAP = 156 * 1024


def plan_with(hook, shapes):
    from new_cg_variants_amd import _lib as L
    n = np.array([s[0] for s in shapes], dtype=np.int64)
    nnz = np.array([s[1] for s in shapes], dtype=np.int64)
    mrl = np.array([s[2] for s in shapes], dtype=np.int32)
    mode, group = np.full(len(shapes), -1, dtype=np.int32), np.full(len(shapes), -1, dtype=np.int32)
    rc = getattr(L.lib(), hook)(len(shapes), L.ptr(n), L.ptr(nnz), L.ptr(mrl), L.ptr(mode), L.ptr(group))
    return rc, mode.tolist(), group.tolist()


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_partitions():
    assert uniform(10, 3).tolist() == [0, 3, 6, 9, 10] and uniform(9, 3).tolist() == [0, 3, 6, 9] and uniform(5, 8).tolist() == [0, 5]
    assert cyclic(40).tolist() == [0, 1, 3, 6, 10, 15, 21, 28, 36, 37, 39, 40]
    assert np.diff(cyclic(112)).max() == 8 and cyclic(112)[-1] == 112


def test_header_and_binding():
    from new_cg_variants_amd import _lib as L
    strip = lambda t: re.sub(r'/\*.*?\*/', '', t, flags=re.S)      # noqa: E731
    text = open(os.path.join(ROOT, 'include', 'prcg.h')).read()
    pub = strip(text)
    test_text = open(os.path.join(ROOT, 'include', 'prcg_test.h')).read()
    tst = strip(test_text)
    lib = L.lib()
    assert re.search(r'\bprcg_batch_begin_block_jacobi\s*\(', pub)
    assert 'prcg_batch_begin_block_jacobi' in L._SIGNATURES and hasattr(lib, 'prcg_batch_begin_block_jacobi')
    assert len(L._SIGNATURES['prcg_batch_begin_block_jacobi'][1]) == 9
    assert re.search(r'\bprcg_plan_small_batch_blocks\s*\(', tst) and 'prcg_plan_small_batch_blocks' not in pub
    assert 'prcg_plan_small_batch_blocks' in L._SIGNATURES and hasattr(lib, 'prcg_plan_small_batch_blocks')
    assert L._SIGNATURES['prcg_plan_small_batch_blocks'] == L._SIGNATURES['prcg_plan_small_batch_jacobi']
    assert lib.prcg_version() == 1
    section = text[text.index('a BATCH of small independent systems'):text.index('typedef struct prcg_batch')]
    flat = re.sub(r'\s*\n \*\s*', ' ', section)
    for phrase in ('prcg_batch_begin_block_jacobi',
                   'PACKED format of prcg_set_block_jacobi_var',                     # the packed format
                   'm_k x m_k doubles, row-major, no padding',
                   'zero-based PER SYSTEM, first entry 0, last entry n_s',
                   'acc = B[a][0] * v[start]', 'B[a][j] * v[start+j] for j ascending', 'no FMA',      # the apply loop
                   'VarBlockJacobi.__call__ and BlockJacobi.__call__',
                   'every block of size 1 and inv_blocks = d',                         # the invariant
                   'prcg_batch_begin, prcg_batch_begin_jacobi and prcg_batch_begin_block_jacobi',      # the stop serves it
                   'nblk_off not from 0 or decreasing', 'first entry is not 0 or whose last is not n_s',      # the refusals
                   'a block size outside 1..8', 'a system that does not fit', 'a null pointer',
                   '32 n + 640 + 12 nnz + 16 <= 159744 bytes', 'PRCG_VEC_RT'):
        assert phrase in flat, phrase
    # the rule of the hook, in bytes
    assert '32 n + 640 + 12 nnz + 16 <= 159744 bytes' in re.sub(r'\s*\n \*\s*', ' ', test_text)


def test_planner_hook_under_this_calls_fit_rule(matrices):
    """The exchange between a block's rows adds no LDS (it goes through the buffer of the next iterate's pairs), so this call's
    rule IS the Jacobi rule: the two hooks agree on every shape, at the cap included; both part from the unpreconditioned rule
    on the same system."""
    blocks, jac, plain = 'prcg_plan_small_batch_blocks', 'prcg_plan_small_batch_jacobi', 'prcg_plan_small_batch'
    for name in ('bcsstk03', 'nos4', 'nos7', 'lap32x32'):
        assert plan_with(blocks, [shape_of(system(matrices, name)[0])]) == (1, [1], [0]), name
    bus = shape_of(system(matrices, '494_bus')[0])
    assert bus[:2] == (494, 1666) and 32 * 494 + 640 + 12 * 1666 + 16 == 36456
    assert plan_with(blocks, [bus]) == (1, [0], [0])
    shapes = [shape_of(system(matrices, name)[0]) for name, _, _ in NINE]
    assert plan_with(blocks, shapes) == plan_with(jac, shapes) == (2, [m for _, _, m in NINE], [0 if m else 1 for _, _, m in NINE])
    big = shape_of(matrices['bcsstk14'][0])
    assert big[:2] == (1806, 63454)
    assert plan_with(blocks, shapes + [big])[0] == plan_with(jac, shapes + [big])[0] == -(9 + 1)
    assert plan_with(blocks, [big])[0] == -1
    # at the cap: 32 * 1500 + 640 + 12 * 9257 + 16 = 159740 fits, one nonzero more does not; the rule without a preconditioner
    # (128 bytes less) takes 9268 -- a system that classifies differently WITH a preconditioner, under either hook
    for nnz, fits in ((9257, True), (9258, False), (9268, False)):
        assert (32 * 1500 + 640 + 12 * nnz + 16 <= CAP) == fits
        assert (plan_with(blocks, [(1500, nnz, 7)])[0] == 1) == fits and (plan_with(jac, [(1500, nnz, 7)])[0] == 1) == fits
        assert plan_with(plain, [(1500, nnz, 7)])[0] == 1
    # every system that fits this rule fits the Jacobi rule (and here the converse): a sweep of shapes around the cap and up to
    # four rows per thread
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = int(rng.integers(1025, 4200))
        shape = (n, int(rng.integers(n, 14000)), int(rng.integers(1, 70)))
        assert plan_with(blocks, [shape]) == plan_with(jac, [shape]), shape
    assert plan_with(blocks, [(4096, 2000, 1)]) == (1, [0], [0]) and plan_with(blocks, [(4097, 2000, 1)])[0] == -1      # four rows per thread
    assert plan_with(blocks, [(1024, 8 * 1024, 8)]) == (1, [1], [0])
    from new_cg_variants_amd import _lib as L
    assert L.lib().prcg_plan_small_batch_blocks(0, None, None, None, None, None) == 0


def test_python_argument_checks_come_before_any_device_call(monkeypatch, matrices):
    import new_cg_variants_amd.callbacks as cbs
    import new_cg_variants_amd.cg_variants as cgv
    from new_cg_variants_amd import device, problems

    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(cgv, 'DeviceBatch', no_device)
    monkeypatch.setattr(cgv, 'DeviceCSR', no_device)
    monkeypatch.setattr(cgv, '_operator', no_device)
    A, b = system(matrices, 'bcsstk03')
    A2 = problems.laplace_2d(8, 8)
    n, n2 = A.shape[0], A2.shape[0]
    d = 1 / A.diagonal()
    var = cgv.VarBlockJacobi(A, cyclic(n))

    class Carrier:
        def __init__(self, **kw):
            self.__dict__.update(kw)

    for name in ('pipe_pr_bpcg_batch', 'pipe_pr_m_bpcg_batch', 'hs_bpcg_batch'):
        f = getattr(cgv, name)
        assert name in cgv.__all__ and f.__name__ == name
        bs, x0s = [b, 2 * b, 3 * b], [np.zeros(n)] * 3
        mixed_bs, mixed_x0s = [b, np.ones(n2)], [np.zeros(n), np.zeros(n2)]
        # what the other batch functions refuse
        with pytest.raises(ValueError, match=r'sequence of 3 matrices, one per right-hand side -- got 2'):
            f([A, A], bs, x0s, 5, preconditioner=cgv.BlockJacobi(A, 3))
        with pytest.raises(ValueError, match=r'x0s must hold 3 vectors, one per system -- got 2'):
            f(A, bs, x0s[:2], 5)
        with pytest.raises(ValueError, match='callback error_A_norm is not served by a batch'):
            f(A, bs, x0s, 5, preconditioner=var, callbacks=[cbs.error_A_norm])
        with pytest.raises(ValueError, match='x_true is not served by a batch'):
            f(A, bs, x0s, 5, x_true=np.ones(n))
        with pytest.raises(ValueError, match=rf'{name}: rtol\[1\] = -1.0'):
            f(A, bs, x0s, 5, preconditioner=var, rtol=[1e-8, -1.0, 0.0])
        # anything that is no block Jacobi, Jacobi, diagonal callable or None
        for prec in ('jacobi', 3.0, Carrier(bs=3), Carrier(block_ptr=cyclic(n))):
            with pytest.raises(ValueError, match='is neither a block-Jacobi object'):
                f(A, bs, x0s, 5, preconditioner=prec)
        for prec in (lambda v: A @ v, lambda v: np.roll(v, 1)):
            with pytest.raises(ValueError, match='is a callable that is not a diagonal scaling'):
                f(A, bs, x0s, 5, preconditioner=prec)
        with pytest.raises(ValueError, match=r'preconditioner\[1\] is a callable that is not a diagonal scaling'):
            f(A, bs, x0s, 5, preconditioner=[var, lambda v: A @ v, None])
        # size mismatches
        with pytest.raises(ValueError, match=r'one preconditioner object for 2 systems of different sizes \[64, 112\]'):
            f([A, A2], mixed_bs, mixed_x0s, 5, preconditioner=cgv.BlockJacobi(A, 3))
        with pytest.raises(ValueError, match=r'preconditioner\[1\] carries a partition of 112 rows, the system has size 64'):
            f([A, A2], mixed_bs, mixed_x0s, 5, preconditioner=[var, var])
        with pytest.raises(ValueError, match=r'preconditioner\[1\] carries inv_blocks of shape \(38, 3, 3\), a system of size 64 with bs = 3 has \(22, 3, 3\)'):
            f([A, A2], mixed_bs, mixed_x0s, 5, preconditioner=[None, cgv.BlockJacobi(A, 3)])
        with pytest.raises(ValueError, match=r'preconditioner\[1\] carries a diagonal of shape \(112,\), the system has size 64'):
            f([A, A2], mixed_bs, mixed_x0s, 5, preconditioner=[cgv.Jacobi(A), cgv.Jacobi(A)])
        with pytest.raises(ValueError, match=r'carries 5 entries of inv_blocks, its partition needs'):
            f(A, bs, x0s, 5, preconditioner=Carrier(block_ptr=cyclic(n), inv_blocks=np.ones(5)))
        # a partition the library would refuse
        with pytest.raises(ValueError, match=r'block 1 has size 9, outside 1..8'):
            f(A, bs, x0s, 5, preconditioner=Carrier(block_ptr=[0, 3, 12, n], inv_blocks=np.ones(9)))
        with pytest.raises(ValueError, match=r'block_ptr\[0\] is 1, not 0'):
            f(A, bs, x0s, 5, preconditioner=Carrier(block_ptr=[1, 3, n], inv_blocks=np.ones(9)))
        with pytest.raises(ValueError, match=r'has block size 9, outside 1..8'):
            f(A, bs, x0s, 5, preconditioner=Carrier(bs=9, inv_blocks=np.ones((13, 9, 9))))
        # a sequence of the wrong length
        with pytest.raises(ValueError, match=r'one object or a sequence of 3, one per system -- got 2'):
            f(A, bs, x0s, 5, preconditioner=[var] * 2)
        # what IS served gets as far as the device
        for prec in (None, var, cgv.BlockJacobi(A, 3), cgv.BlockJacobi(A, 8), cgv.Jacobi(A), lambda v: d * v, Carrier(bs=1, inv_blocks=d.reshape(-1, 1, 1)),
                     Carrier(block_ptr=var.block_ptr, inv_blocks=var.inv_blocks), [cgv.BlockJacobi(A, 3), None, var], (None, None, None)):
            with pytest.raises(AssertionError, match='the device was reached'):
                f(A, bs, x0s, 5, preconditioner=prec, callbacks=[cbs.updated_residual_2_norm], rtol=1e-8)
        with pytest.raises(AssertionError, match='the device was reached'):
            f([A, A2], mixed_bs, mixed_x0s, 5, preconditioner=[var, cgv.BlockJacobi(A2, 2)])
        with pytest.raises(AssertionError, match='the device was reached'):
            f([A, A2], mixed_bs, mixed_x0s, 5)
    # what a batch is begun with
    got = cgv._batch_blocks('f', [cgv.BlockJacobi(A, 3), var, None, cgv.Jacobi(A), lambda v: d * v], [n] * 5)
    u3 = cgv.VarBlockJacobi(A, uniform(n, 3))
    assert np.array_equal(got[0][0], uniform(n, 3)) and got[0][1].shape == (37 * 9 + 1,) and np.array_equal(got[0][1], u3.inv_blocks)
    assert np.array_equal(cgv.BlockJacobi(A, 3)(b), u3(b))       # ... and the uniform object applies what the partition's does
    assert got[1][0] is var.block_ptr or np.array_equal(got[1][0], var.block_ptr)
    assert np.array_equal(got[1][1], var.inv_blocks)
    for (ptr, inv), want in zip(got[2:], (np.ones(n), d, d)):
        assert np.array_equal(ptr, np.arange(n + 1)) and np.array_equal(inv, want)
    # the diagonal batch functions still refuse block objects, with their old message
    with pytest.raises(ValueError, match='a batch applies diagonal preconditioners only'):
        cgv.pipe_pr_pcg_batch(A, bs, x0s, 5, preconditioner=cgv.BlockJacobi(A, 2))
    # DeviceBatch.begin: one preconditioner; its block_jacobi shaped on the host
    with pytest.raises(ValueError, match='inv_diag and block_jacobi are mutually exclusive'):
        device.DeviceBatch.begin(None, 0, [], [], 5, inv_diag=[d], block_jacobi=[(var.block_ptr, var.inv_blocks)])
    with pytest.raises(ValueError, match=r'block_jacobi must hold 2 pairs \(block_ptr, inv_blocks\), one per system -- got 1'):
        device.batch_blocks('block_jacobi', [(var.block_ptr, var.inv_blocks)], [n, n])
    with pytest.raises(ValueError, match=r'block_jacobi\[1\]: inv_blocks holds 4 entries, the partition\'s blocks have 112'):
        device.batch_blocks('block_jacobi', [(var.block_ptr, var.inv_blocks), (np.arange(n + 1), np.ones(4))], [n, n])
    with pytest.raises(ValueError, match=r'block_jacobi\[0\] must be a pair'):
        device.batch_blocks('block_jacobi', [3.0], [n])
    off, ptr, inv = device.batch_blocks('block_jacobi', [(var.block_ptr, var.inv_blocks), (np.arange(n + 1), d)], [n, n])
    nb = var.block_ptr.size - 1
    assert off.tolist() == [0, nb, nb + n] and off.dtype == ptr.dtype == np.int64 and ptr.size == nb + n + 2
    assert np.array_equal(ptr[off[1] + 1:], np.arange(n + 1)) and np.array_equal(inv, np.concatenate([var.inv_blocks, d]))
    import inspect
    assert inspect.signature(device.DeviceBatch.begin).parameters['block_jacobi'].default is None


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def amd():
    import new_cg_variants_amd.callbacks as cbs
    import new_cg_variants_amd.cg_variants as cgv
    from new_cg_variants_amd import _lib, device, problems
    return dict(cgv=cgv, cbs=cbs, L=_lib, device=device, problems=problems)


@pytest.fixture(scope='module')
def ten(matrices):
    systems, precs, mats, mat_of = ten_systems(matrices)
    assert len(mats) == 5 and mat_of == [0, 0, 0, 1, 2, 2, 3, 3, 4, 4]      # systems on one matrix, different partitions
    return dict(systems=systems, precs=precs, mats=mats, mat_of=mat_of, thr=thresholds([b for _, b in systems], rtol=RTOL))


@pytest.fixture(scope='module')
def oracle(ten):
    """variant -> [(run, halt)] of the ten systems: computed once, never modified"""
    cache = {}

    def get(variant):
        if variant not in cache:
            cache[variant] = [trajectory(A, b, variant, p, t) for (A, b), p, t in zip(ten['systems'], ten['precs'], ten['thr'])]
        return cache[variant]
    return get


@pytest.fixture(scope='module')
def base(amd, ten):
    """variant -> the device records of the ten systems, 60 iterations cut at k = 1: computed once, never modified"""
    cache = {}

    def get(variant):
        if variant not in cache:
            cache[variant] = run_blocks(amd, ten['systems'], variant, blocks_of(ten['precs']), (1, FREE - 1), mat_of=ten['mat_of'],
                                        matrices=ten['mats'])
        return cache[variant]
    return get


def free_want(run, total):
    """a run without thresholds in the form holds_oracle takes"""
    return dict(k_stop=-1, status=0, last=total, at0=run['vec'][0], at=run['vec'][total], scalars=run['scalars'], coef=run['coef'],
                hist=run['hist'])


def holds_run(rec, run, variant, total, what, at=(0, 1)):
    idx = slots(variant)
    assert np.all(np.isfinite(run['scalars'][:, idx])) and np.all(run['scalars'][:, [0, 3, 4]] != 0), (what, 'the oracle breaks down')
    holds_oracle(rec, free_want(run, total), variant, total, what)
    for k in at:
        for v in run['vec'][k]:
            assert np.array_equal(rec['vec'][k][v], run['vec'][k][v]), (what, k, v)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_whole_trajectory_against_the_oracle(ten, oracle, base, variant):
    for case, rec, (run, _) in zip(TEN, base(variant), oracle(variant)):
        holds_run(rec, run, variant, FREE, (variant,) + case)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_every_system_stops_where_the_oracle_does(amd, ten, oracle, variant):
    total = MAX_ITER - 1
    halts = [h for _, h in oracle(variant)]
    assert any(h['status'] == CONVERGED and 0 < h['k_stop'] < total for h in halts)
    assert all(h['status'] in (CONVERGED, BREAKDOWN) and 0 < h['k_stop'] < total for h in halts), [h['k_stop'] for h in halts]
    if variant != 'HS':
        assert halts[NOS7_BS8]['status'] == BREAKDOWN
    recs = run_blocks(amd, ten['systems'], variant, blocks_of(ten['precs']), (100, total - 100), rr_stop=ten['thr'], mat_of=ten['mat_of'],
                      matrices=ten['mats'], max_iter=MAX_ITER)
    for case, rec, halt in zip(TEN, recs, halts):
        holds_oracle(rec, halt, variant, total, (variant,) + case)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_a_partition_of_ones_is_the_jacobi_batch(amd, matrices, variant):
    nine = [system(matrices, name) for name, _, _ in NINE]
    d = jacobi_of(nine)
    ones = run_blocks(amd, nine, variant, [(np.arange(A.shape[0] + 1), q) for (A, _), q in zip(nine, d)], (1, FREE - 1))
    jac = run_blocks(amd, nine, variant, None, (1, FREE - 1), inv_diag=d)
    for (name, _, _), a, b in zip(NINE, ones, jac):
        assert np.all(np.isfinite(b['hist'][:10])) and b['hist'][0] > 0, name
        same_record(a, b, (variant, name))


def straddlers(amd):
    """Blocks across a thread's rows (row = tid + j * 1024), all with the matrix in LDS: lap33x32 bs 3 (block 341 owns rows 1023..1025),
    lap40x40 bs 7 (block 146 owns 1022..1028); n = 2100 tridiagonal, bs 3 (block 682 owns 2046..2048, a third row in 52 threads);
    n = 3080 coupled for i >= 2180, bs 7 (block 438 owns 3066..3072, a fourth row in 8 threads; 146 and 292 straddle too).  The
    oracle's stops at rtol = 3e-2, asserted below to lie strictly inside the 12 iterations: 8, 3, 3, 3."""
    lap = amd['problems'].laplace_2d

    def rhs(n):                                                  # oscillating: under ones no stop lies inside 12 iterations
        i = np.arange(n)
        return (-1.0) ** i + 0.25 * np.sin(0.37 * i)
    out = [((lap(33, 32), rhs(1056)), 3), ((lap(40, 40), rhs(1600)), 7), (tall_system(2100, 0), 3), (tall_system(3080, 2180), 7)]
    for ((A, _), bs), row in zip(out, (1023, 1023, 2047, 3071)):
        ptr = uniform(A.shape[0], bs)
        k = np.searchsorted(ptr, row, side='right') - 1
        assert ptr[k] <= row < row + 1 < ptr[k + 1], (bs, row)       # rows `row` and `row + 1` share a block
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_blocks_across_a_threads_rows(amd, variant):
    iters = 12
    cases = straddlers(amd)
    systems = [sb for sb, _ in cases]
    rc, mode, _ = plan_with('prcg_plan_small_batch_blocks', [shape_of(A) for A, _ in systems])
    assert rc == 1 and mode == [0, 0, 0, 0]
    precs = [amd['cgv'].VarBlockJacobi(A, uniform(A.shape[0], bs)) for (A, _), bs in cases]
    thr = thresholds([b for _, b in systems], rtol=3e-2)
    both = [trajectory(A, b, variant, p, t, free=iters, cap=iters) for (A, b), p, t in zip(systems, precs, thr)]
    recs = run_blocks(amd, systems, variant, blocks_of(precs), (1, iters - 1))
    halted = run_blocks(amd, systems, variant, blocks_of(precs), (iters,), rr_stop=thr)
    for s, ((run, halt), rec, got) in enumerate(zip(both, recs, halted)):
        holds_run(rec, run, variant, iters, (variant, s))
        assert halt['status'] == CONVERGED and 0 < halt['k_stop'] < iters, (variant, s, halt['k_stop'])      # strictly inside the run
        holds_oracle(got, halt, variant, iters, (variant, s, 'stopped'))


def same_common(a, b, what):
    """two records of runs cut at different places: what both hold"""
    last = max(a['vec'])
    assert last == max(b['vec'])
    a, b = dict(a), dict(b)
    a['vec'], b['vec'] = {k: a['vec'][k] for k in (0, last)}, {k: b['vec'][k] for k in (0, last)}
    same_record(a, b, what)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_cutting_order_and_company_change_nothing(amd, ten, base, variant):
    want = base(variant)
    systems, blocks, mats, mat_of = ten['systems'], blocks_of(ten['precs']), ten['mats'], ten['mat_of']
    cut = run_blocks(amd, systems, variant, blocks, (20, 1, 39), mat_of=mat_of, matrices=mats)
    for case, a, b in zip(TEN, cut, want):
        same_common(a, b, ('cut',) + case)
    rev = run_blocks(amd, systems[::-1], variant, blocks[::-1], (FREE,), mat_of=mat_of[::-1], matrices=mats)[::-1]
    for case, a, b in zip(TEN, rev, want):
        same_common(a, b, ('reversed',) + case)
    for members in ([8, 9], [2, 5], [7]):                        # the LDS group alone; two and one of the register group
        part = run_blocks(amd, [systems[i] for i in members], variant, [blocks[i] for i in members], (FREE,))
        for i, a in zip(members, part):
            same_common(a, want[i], ('alone',) + TEN[i])


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['PIPE_PR', 'HS'])
def test_more_systems_than_cus_on_one_matrix(amd, ten, base, variant):
    """B = 300 of bcsstk03, the three partitions in turn: system s carries the bits of system s mod 3 of the ten"""
    n_sys = 300
    (A, b), blocks = ten['systems'][0], blocks_of(ten['precs'][:3])
    n = A.shape[0]
    batch = amd['device'].DeviceBatch([A], np.zeros(n_sys, dtype=np.int32))
    try:
        batch.begin(getattr(amd['L'], variant), np.tile(b, (n_sys, 1)), np.zeros((n_sys, n)), FREE + 1, hist_mask=1,
                    block_jacobi=[blocks[s % 3] for s in range(n_sys)])
        batch.iterate(FREE)
        batch.sync()
        X = batch.solutions().reshape(n_sys, n)
        hists = np.array([batch.history(s)['updated_residual_2_norm'] for s in range(n_sys)])
    finally:
        batch.close()
    for s in range(n_sys):
        want = base(variant)[s % 3]
        assert np.array_equal(X[s], want['at']['x']) and np.array_equal(hists[s], want['hist']), s
    assert not np.array_equal(X[0], X[1]) and not np.array_equal(X[1], X[2])


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_a_poisoned_block_stays_in_its_system(amd, ten, base, variant):
    """a nan in one entry of one block of system 4 (nos7, bs 3): r~ = M^-1 r is nan in that block from the start, so row 0 has nan
    in mu and nu while rr_0 = r.r is the clean run's; every later history entry is nan.  Every other system is untouched."""
    want = base(variant)
    blocks = [(ptr, inv.copy()) for ptr, inv in blocks_of(ten['precs'])]
    blocks[4][1][9 * 17 + 4] = np.nan
    got = run_blocks(amd, ten['systems'], variant, blocks, (FREE,), mat_of=ten['mat_of'], matrices=ten['mats'])
    for i, (case, a, b) in enumerate(zip(TEN, got, want)):
        if i != 4:
            same_common(a, b, ('poisoned company',) + case)
    row0 = got[4]['scalars'][0]
    assert np.all(np.isnan(row0[[0, 3]])) and got[4]['hist'][0] == want[4]['hist'][0] and np.all(np.isnan(got[4]['hist'][1:]))
    assert np.all(np.isnan(got[4]['at']['x']))


@pytest.mark.gpu
def test_refusals_through_the_c_abi(amd, matrices):
    L = amd['L']
    lib = L.lib()
    A3, b3 = system(matrices, 'bcsstk03')
    A4 = system(matrices, 'nos4')[0]
    n3, n4 = A3.shape[0], A4.shape[0]
    i = np.arange(1500)                              # n = 1500, nnz = 9268: at the cap without a preconditioner, 128 bytes over with one
    lens = np.full(1500, 6)
    lens[:268] += 1
    import scipy.sparse as sp
    indices = np.concatenate([(q + 37 * np.arange(lens[q])) % 1500 for q in i]).astype(np.int32)
    near = sp.csr_matrix((np.where(indices == np.repeat(i, lens), 10.0, 1.0), indices, np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)),
                         shape=(1500, 1500))
    assert near.nnz == 9268
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
    fn = 'prcg_batch_begin_block_jacobi'
    try:
        sizes = [n3, n4, n3]
        bt = create([A3, A4], [0, 1, 0])
        try:
            n_all = sum(sizes)
            rhs, x0 = np.ones(n_all), np.zeros(n_all)
            ptrs = [uniform(n3, 3), cyclic(n4), uniform(n3, 8)]
            off = np.concatenate([[0], np.cumsum([p.size - 1 for p in ptrs])]).astype(np.int64)
            ptr = np.concatenate(ptrs)
            inv = np.full(int(sum(np.sum(np.diff(p) ** 2) for p in ptrs)), 0.5)

            def begin_refused(text, variant=L.PIPE_PR, r=rhs, x=x0, o=off, p=ptr, b=inv, max_iter=5, mask=1):
                rc = lib.prcg_batch_begin_block_jacobi(bt, variant, L.ptr(r), L.ptr(x), L.ptr(o), L.ptr(p), L.ptr(b), max_iter, mask)
                assert rc == L.EINVAL and re.search(text, error()), (rc, error())

            def changed(at, value, base=ptr):
                q = base.copy()
                q[at] = value
                return q
            # an open session, which every refusal must leave alone
            assert lib.prcg_batch_begin_jacobi(bt, L.HS, L.ptr(rhs), L.ptr(x0), L.ptr(np.ones(n_all)), 5, 1) == L.OK
            assert lib.prcg_batch_iterate(bt, 2) == L.OK
            for variant in (L.PIPE_P, L.PIPE_P_M, L.PR, L.M, L.CG_CG, L.GV, 99, -1):
                begin_refused(rf'{fn}: variant {variant} is not served by a batch', variant=variant)
            for mask in (2, 4, 8, 3, 16):
                begin_refused(rf'{fn}: history bits {mask}', mask=mask)
            for key in ('r', 'x', 'o', 'p', 'b'):
                begin_refused(rf'{fn}: null rhs, x0, nblk_off, block_ptr or inv_blocks', **{key: None})
            begin_refused(rf'{fn}: max_iter = 0', max_iter=0)
            begin_refused(rf'{fn}: max_iter = -3', max_iter=-3)
            begin_refused(rf'{fn}: nblk_off\[0\] is 1, not 0', o=changed(0, 1, off))
            begin_refused(rf'{fn}: nblk_off decreases at system 1', o=changed(2, off[1] - 1, off))
            s1 = int(off[1]) + 1                         # first entry of system 1's partition
            begin_refused(rf'{fn}: the partition of system 1 starts at 1, not 0', p=changed(s1, 1))
            begin_refused(rf'{fn}: the partition of system 0 ends at 111, not at its n = 112', p=changed(s1 - 1, 111))
            begin_refused(rf'{fn}: the partition of system 2 ends at {n3 + 1}, not at its n = 112', p=changed(-1, n3 + 1))
            begin_refused(rf'{fn}: system 0, block 1 has size 9, outside 1..8', p=changed(2, 12))
            begin_refused(rf'{fn}: system 1, block 2 has size 0, outside 1..8', p=changed(s1 + 3, 3))
            begin_refused(rf'{fn}: system 1, block 1 has size -1, outside 1..8', p=changed(s1 + 2, 0))
            # ... nothing was changed: the session goes on
            assert lib.prcg_batch_iteration(bt) == 2 and lib.prcg_batch_iterate(bt, 2) == L.OK and lib.prcg_batch_sync(bt) == L.OK
            assert lib.prcg_batch_iteration(bt) == 4
            hist = np.zeros(5)
            assert lib.prcg_batch_get_history(bt, 1, L.ptr(hist)) == L.OK and np.all(np.isfinite(hist)) and hist[0] > 0
            # ... and the same object begins a block session, whose r~ = M^-1 r is readable where it is held
            assert lib.prcg_batch_begin_block_jacobi(bt, L.PIPE_PR_M, L.ptr(rhs), L.ptr(x0), L.ptr(off), L.ptr(ptr), L.ptr(inv), 5, 1) == L.OK
            rt, r = np.full(n4, -1.0), np.full(n4, -1.0)
            assert lib.prcg_batch_get_vector(bt, L.VEC['rt'], 1, L.ptr(rt)) == L.OK and lib.prcg_batch_get_vector(bt, L.VEC['r'], 1, L.ptr(r)) == L.OK
            assert np.array_equal(r, np.ones(n4)) and np.array_equal(rt[:6], [0.5, 1.0, 1.0, 1.5, 1.5, 1.5])      # blocks of 0.5: m / 2
            assert lib.prcg_batch_begin_block_jacobi(bt, L.HS, L.ptr(rhs), L.ptr(x0), L.ptr(off), L.ptr(ptr), L.ptr(inv), 5, 1) == L.OK
            assert lib.prcg_batch_get_vector(bt, L.VEC['rt'], 1, L.ptr(rt)) == L.EINVAL and re.search('this session is Hestenes-Stiefel', error())
            assert lib.prcg_batch_iterate(bt, 4) == L.OK and lib.prcg_batch_sync(bt) == L.OK and lib.prcg_batch_iteration(bt) == 4
        finally:
            lib.prcg_batch_destroy(bt)
        # ---- a system that does not fit this call's rule: the first such system is named
        bt = create([A3, near], [0, 1])
        try:
            n_all = n3 + 1500
            rhs, x0 = np.ones(n_all), np.zeros(n_all)
            off = np.array([0, n3, n_all], dtype=np.int64)
            ptr = np.concatenate([np.arange(n3 + 1), np.arange(1501)]).astype(np.int64)
            assert lib.prcg_batch_begin(bt, L.PIPE_PR, L.ptr(rhs), L.ptr(x0), 5, 1) == L.OK and lib.prcg_batch_iterate(bt, 2) == L.OK
            for variant in (L.PIPE_PR, L.PIPE_PR_M, L.HS):
                rc = lib.prcg_batch_begin_block_jacobi(bt, variant, L.ptr(rhs), L.ptr(x0), L.ptr(off), L.ptr(ptr), L.ptr(np.ones(n_all)), 5, 1)
                assert rc == L.EINVAL and re.search(rf'{fn}: system 1 \(n = 1500, nnz = 9268\) fits the one-workgroup solver without a '
                                                    r'preconditioner but not with one: the preconditioned solver needs 159872 bytes', error()), error()
            assert lib.prcg_batch_iteration(bt) == 2 and lib.prcg_batch_iterate(bt, 2) == L.OK and lib.prcg_batch_sync(bt) == L.OK
        finally:
            lib.prcg_batch_destroy(bt)
        # after all the refusals the handle still serves an ordinary single session
        op.begin(L.PIPE_PR, b3, np.zeros(b3.size), 21, hist_mask=1)
        op.iterate(20)
        hist = op.history()['updated_residual_2_norm']
        assert np.all(np.isfinite(hist[:20])) and hist[0] > 0
    finally:
        op.close()
    # the Python object reports the library's text
    batch = amd['device'].DeviceBatch([A3])
    try:
        with pytest.raises(L.PrcgError, match=r'system 0, block 0 has size 9, outside 1..8'):
            batch.begin(L.PIPE_PR, [b3], [np.zeros(n3)], 5, block_jacobi=[(np.array([0, 9, n3 - 7, n3]), np.ones(81 + (n3 - 16) ** 2 + 49))])
    finally:
        batch.close()


@pytest.mark.gpu
def test_the_python_functions(amd, ten, oracle):
    cgv, cbs = amd['cgv'], amd['cbs']
    A0, b0 = ten['systems'][0]                       # bcsstk03
    A1, b1 = ten['systems'][3]                       # nos4
    precs = [cgv.BlockJacobi(A0, 3), cgv.VarBlockJacobi(A1, cyclic(A1.shape[0])), None]
    As, bs = [A0, A1, A0], [b0, b1, b0]
    x0s = [np.zeros(b.size) for b in bs]
    max_iter = 41
    calls = [p if p is not None else (lambda v: np.array(v, copy=True)) for p in precs]      # None is the identity
    wants = [trajectory(A, b, 'PIPE_PR', p, free=max_iter - 1)[0] for A, b, p in zip(As, bs, calls)]
    # (BlockJacobi(A0, 3) carries the inverses of system 0 of the ten: the same trajectory)
    assert np.array_equal(wants[0]['hist'], oracle('PIPE_PR')[0][0]['hist'][:max_iter])
    out = cgv.pipe_pr_bpcg_batch(As, bs, x0s, max_iter, preconditioner=precs, callbacks=[cbs.updated_residual_2_norm])
    assert len(out) == 3
    for s, (trial, want) in enumerate(zip(out, wants)):
        assert trial['name'] == 'pipe_pr_bpcg_batch' and trial['max_iter'] == max_iter and trial['system'] == s
        assert 'iterations' not in trial and 'status' not in trial
        assert np.all(np.isfinite(want['hist'])) and np.array_equal(trial['updated_residual_2_norm'], want['hist']), s
    for fn, variant in (('pipe_pr_bpcg_batch', 'PIPE_PR'), ('pipe_pr_m_bpcg_batch', 'PIPE_PR_M'), ('hs_bpcg_batch', 'HS')):
        thr = thresholds(bs, rtol=1e-3)
        halts = [trajectory(A, b, variant, p, t, free=0, cap=max_iter - 1)[1] for A, b, p, t in zip(As, bs, calls, thr)]
        out = getattr(cgv, fn)(As, bs, x0s, max_iter, preconditioner=precs, callbacks=[cbs.updated_residual_2_norm], rtol=1e-3)
        for s, (trial, halt) in enumerate(zip(out, halts)):
            status = ('max_iter', 'converged', 'breakdown')[halt['status']]
            assert (trial['iterations'], trial['status']) == (halt['last'], status), (fn, s, trial['iterations'], trial['status'])
            hist = np.zeros(max_iter)
            hist[:halt['last'] + 1] = halt['hist']
            assert np.array_equal(trial['updated_residual_2_norm'], hist), (fn, s)
        assert {t['status'] for t in out} >= {'converged'}, fn
