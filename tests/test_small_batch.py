"""A batch of small independent systems solved in one launch, one workgroup per system (prcg.h: prcg_batch_create;
device.DeviceBatch; cg_variants.*_batch).

CPU: the planner hook's classification, the Python argument checks, header and binding.
GPU: every system of a batch carries the bits of the single one-workgroup solver (forced from the batch's own initial inner
products, whose summation order is the workgroup's and may differ from the single session's start-up launches in the last
bit), whatever its position, group or company; cutting; a shared matrix with more systems than CUs; isolation of a NaN; the
oracle's golden histories; the refusals of the C-ABI; the reference-shaped functions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_run
from small_batch_common import NINE, VARIANTS, csr_cat, plan, shape_of, slots, system

ITERS = 200


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_planner_classifies_the_nine_systems(matrices):
    from new_cg_variants_amd import problems
    shapes = []
    for name, n, _ in NINE:
        A, _b = system(matrices, name)
        assert A.shape[0] == n
        shapes.append(shape_of(A))
    rc, mode, group = plan(shapes)
    assert rc == 2
    assert mode.tolist() == [m for _, _, m in NINE]
    assert group.tolist() == [0 if m == 1 else 1 for _, _, m in NINE]        # the register group is launched first
    # a system that does not fit: its index, as -(s + 1)
    big = shape_of(matrices['bcsstk14'][0])
    assert big[1] == 63454
    assert plan(shapes + [big])[0] == -(9 + 1)
    assert plan(shapes[:4] + [shape_of(problems.laplace_2d(64, 64))] + shapes[4:] + [big])[0] == -(4 + 1)
    # a permutation of the systems permutes the modes and leaves the number of groups alone
    perm = np.random.default_rng(7).permutation(9)
    rc_p, mode_p, group_p = plan([shapes[i] for i in perm])
    assert rc_p == 2 and mode_p.tolist() == mode[perm].tolist() and group_p.tolist() == group[perm].tolist()
    # one mode only: one group, numbered 0
    rc_1, _, group_1 = plan(shapes[5:])
    assert rc_1 == 1 and set(group_1.tolist()) == {0}


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
    for name in ('pipe_pr_cg_batch', 'pipe_pr_m_cg_batch', 'hs_cg_batch'):
        f = getattr(cgv, name)
        assert name in cgv.__all__ and f.__name__ == name
        bs, x0s = [b, 2 * b, 3 * b], [np.zeros(n)] * 3
        with pytest.raises(ValueError, match=r'sequence of 3 matrices, one per right-hand side -- got 2'):
            f([A, A], bs, x0s, 5)
        with pytest.raises(ValueError, match=r'x0s must hold 3 vectors, one per system -- got 2'):
            f(A, bs, x0s[:2], 5)
        with pytest.raises(ValueError, match=rf'bs\[1\] must have shape \({n2},\), the size of system 1'):
            f([A, A2, A], bs, x0s, 5)
        with pytest.raises(ValueError, match=r'2-D array of shape \(2, 112\) but the systems have different sizes'):
            f([A, A2], np.ones((2, n)), [np.zeros(n), np.zeros(n2)], 5)
        with pytest.raises(ValueError, match=rf'bs must have shape \(3, {n}\)'):
            f(A, np.ones((3, n + 1)), np.zeros((3, n)), 5)
        with pytest.raises(ValueError, match='callback error_A_norm is not served by a batch'):
            f(A, bs, x0s, 5, callbacks=[cbs.error_A_norm])
        with pytest.raises(ValueError, match='is not served by a batch'):
            f(A, bs, x0s, 5, callbacks=[lambda **env: None])
        with pytest.raises(ValueError, match='takes no preconditioner'):
            f(A, bs, x0s, 5, preconditioner=cgv.Jacobi(A))
        # what IS served gets as far as the device: lists and a 2-D array
        with pytest.raises(AssertionError, match='the device was reached'):
            f(A, bs, x0s, 5, callbacks=[cbs.updated_residual_2_norm])
        with pytest.raises(AssertionError, match='the device was reached'):
            f([A, A2], [b, np.ones(n2)], [np.zeros(n), np.zeros(n2)], 5)
        with pytest.raises(AssertionError, match='the device was reached'):
            f(A, np.ones((4, n)), np.zeros((4, n)), 5)


def test_same_object_shares_one_matrix():
    from new_cg_variants_amd import device, problems
    A, B = problems.laplace_2d(5, 5), problems.laplace_2d(5, 5)
    mats, mat_of = device.batch_matrices([A, B, A, A, B])
    assert [m is q for m, q in zip(mats, (A, B))] == [True, True] and mat_of == [0, 1, 0, 0, 1]
    mats, mat_of = device.batch_matrices(A, 3)
    assert mats[0] is A and mat_of == [0, 0, 0]


def test_header_and_binding():
    from new_cg_variants_amd import _lib as L
    names = ['prcg_batch_create', 'prcg_batch_destroy', 'prcg_batch_begin', 'prcg_batch_iterate', 'prcg_batch_sync', 'prcg_batch_iteration',
             'prcg_batch_get_vector', 'prcg_batch_get_solutions', 'prcg_batch_get_scalars', 'prcg_batch_get_coefficients',
             'prcg_batch_get_history']
    strip = lambda t: re.sub(r'/\*.*?\*/', '', t, flags=re.S)      # noqa: E731
    pub = strip(open(os.path.join(ROOT, 'include', 'prcg.h')).read())
    tst = strip(open(os.path.join(ROOT, 'include', 'prcg_test.h')).read())
    lib = L.lib()
    for name in names:
        assert re.search(rf'\b{name}\s*\(', pub), name
        assert name in L._SIGNATURES and hasattr(lib, name), name
    assert re.search(r'\bprcg_plan_small_batch\s*\(', tst) and 'prcg_plan_small_batch' not in pub
    assert 'prcg_plan_small_batch' in L._SIGNATURES and hasattr(lib, 'prcg_plan_small_batch')
    assert lib.prcg_version() == 1
    # the header says what the entries replace in the reference
    text = open(os.path.join(ROOT, 'include', 'prcg.h')).read()
    section = text[text.index('a BATCH of small independent systems'):text.index('typedef struct prcg_batch')]
    for word in ('figure_gen.py:59', ':245-339', 'PRCG_PIPE_PR', 'PRCG_HS', 'DESIGN.md section 4'):
        assert word in section, word


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def amd():
    import new_cg_variants_amd.callbacks as cbs
    import new_cg_variants_amd.cg_variants as cgv
    from new_cg_variants_amd import _lib, device, problems
    return dict(cgv=cgv, cbs=cbs, L=_lib, device=device, problems=problems)


def read_system(op, s, iters, variant, begin=None):
    """everything a session holds for one system; op: a DeviceBatch (s: the system) or a DeviceCSR (s None)"""
    at = () if s is None else (s,)
    out = dict(begin or {})
    for v in ('x', 'r', 'p', 's'):
        out[v] = op.get_vector(v, *at)
    out['scalars'] = np.array([op.get_scalars(k, *at)[slots(variant)] for k in range(1, iters + 1)])
    out['coef'] = np.array([op.get_coefficients(k, *at) for k in range(1, iters + 1)])
    out['hist'] = (op.history(*at) if s is not None else op.history())['updated_residual_2_norm']
    return out


def read_begin(op, s):
    at = () if s is None else (s,)
    out = {'begin_' + v: op.get_vector(v, *at) for v in ('x', 'r', 'p', 's')}
    out['row0'] = op.get_scalars(0, *at)
    return out


def run_batch(amd, systems, variant, chunks=(ITERS,), max_iter=ITERS + 1, mat_of=None, matrices=None):
    """one DeviceBatch session over `systems` [(A, b)]; returns one record per system"""
    L = amd['L']
    mats = [A for A, _ in systems] if matrices is None else matrices
    batch = amd['device'].DeviceBatch(mats, mat_of)
    try:
        batch.begin(getattr(L, variant), [b for _, b in systems], [np.zeros(b.size) for _, b in systems], max_iter, hist_mask=1)
        begins = [read_begin(batch, s) for s in range(len(systems))]
        for c in chunks:
            batch.iterate(c)
        batch.sync()
        assert batch.k == sum(chunks)
        return [read_system(batch, s, sum(chunks), variant, begins[s]) for s in range(len(systems))]
    finally:
        batch.close()


def same(a, b, what=''):
    for key in ('begin_x', 'begin_r', 'begin_p', 'begin_s', 'row0', 'x', 'r', 'p', 's', 'scalars', 'coef', 'hist'):
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key], equal_nan=True), (what, key)


@pytest.fixture(scope='module')
def nine(matrices):
    return [system(matrices, name) for name, _, _ in NINE]


@pytest.fixture(scope='module')
def base(amd, nine):
    """variant -> the records of the nine systems in one batch, 200 iterations in one call: computed once, never modified"""
    cache = {}

    def get(variant):
        if variant not in cache:
            cache[variant] = run_batch(amd, nine, variant)
        return cache[variant]
    return get


def forced_single(amd, A, b, variant, rec, iters):
    """a single session on A, forced to the batch's row-0 scalars, must hold the record's bits"""
    L = amd['L']
    op = amd['device'].DeviceCSR(A)
    try:
        op.begin(getattr(L, variant), b, np.zeros(b.size), iters + 1, hist_mask=1)
        assert op.schedule()['small']
        for v in ('x', 'r', 'p', 's'):
            assert np.array_equal(op.get_vector(v), rec['begin_' + v], equal_nan=True), ('begin', v)
        idx = slots(variant)
        mine, theirs = op.get_scalars(0)[idx], rec['row0'][idx]
        print('row 0, single vs batch, relative:', np.abs(mine - theirs) / np.abs(mine))
        assert np.all(np.abs(mine - theirs) <= 1e-12 * np.abs(mine))
        op.set_scalars(0, rec['row0'])
        op.set_iteration(0)
        op.iterate(iters)
        op.sync()
        got = read_system(op, None, iters, variant)
        for key in ('x', 'r', 'p', 's', 'scalars', 'coef', 'hist'):
            assert got[key].shape == rec[key].shape and np.array_equal(got[key], rec[key], equal_nan=True), key
    finally:
        op.close()


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_every_system_carries_the_single_solvers_bits(amd, nine, base, variant):
    recs = base(variant)
    for (name, n, _), (A, b), rec in zip(NINE, nine, recs):
        assert rec['x'].shape == (n,) and rec['scalars'].shape == (ITERS, len(slots(variant))) and rec['hist'].shape == (ITERS + 1,)
        assert np.all(np.isfinite(rec['hist'][:5])) and rec['hist'][0] > 0, name
        forced_single(amd, A, b, variant, rec, ITERS)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_cutting_the_run_changes_nothing(amd, nine, base, variant):
    cut = run_batch(amd, nine, variant, chunks=(100, 1, 99))
    for (name, _, _), a, b in zip(NINE, cut, base(variant)):
        same(a, b, name)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_order_and_grouping_do_not_matter(amd, nine, base, variant):
    want = base(variant)
    rev = run_batch(amd, nine[::-1], variant)[::-1]
    for (name, _, _), a, b in zip(NINE, rev, want):
        same(a, b, 'reversed ' + name)
    for mode in (1, 0):
        members = [i for i, (_, _, m) in enumerate(NINE) if m == mode]
        part = run_batch(amd, [nine[i] for i in members], variant)
        for i, a in zip(members, part):
            same(a, want[i], f'mode {mode} alone: ' + NINE[i][0])


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['PIPE_PR', 'HS'])
def test_shared_matrix_and_more_systems_than_cus(amd, matrices, variant):
    L = amd['L']
    A, b = system(matrices, 'bcsstk03')
    n, n_sys, iters = A.shape[0], 300, 50
    B = np.array([b * (1 + s % 7) for s in range(n_sys)])
    batch = amd['device'].DeviceBatch([A], np.zeros(n_sys, dtype=np.int32))
    try:
        batch.begin(getattr(L, variant), B, np.zeros((n_sys, n)), iters + 1, hist_mask=1)
        begins = {s: read_begin(batch, s) for s in (0, 151, 299)}
        batch.iterate(iters)
        batch.sync()
        X = batch.solutions()
        assert X.shape == (n_sys * n,)
        xs = np.array([batch.get_vector('x', s) for s in range(n_sys)])
        assert np.array_equal(X, xs.reshape(-1), equal_nan=True)
        hists = np.array([batch.history(s)['updated_residual_2_norm'] for s in range(n_sys)])
        for c in range(7):
            assert np.array_equal(xs[c::7], np.broadcast_to(xs[c], xs[c::7].shape), equal_nan=True), c
            assert np.array_equal(hists[c::7], np.broadcast_to(hists[c], hists[c::7].shape), equal_nan=True), c
        assert not np.array_equal(xs[0], xs[1])
        recs = {s: read_system(batch, s, iters, variant, begins[s]) for s in (0, 151, 299)}
    finally:
        batch.close()
    for s, rec in recs.items():
        forced_single(amd, A, B[s], variant, rec, iters)


@pytest.mark.gpu
@pytest.mark.parametrize('variant', VARIANTS)
def test_a_nan_stays_in_its_system(amd, nine, base, variant):
    poisoned = [(A, b.copy()) for A, b in nine]
    poisoned[3][1][5] = np.nan
    got = run_batch(amd, poisoned, variant)
    assert np.all(np.isnan(got[3]['hist'])), 'the history of system 3 is NaN from index 0'
    for i, ((name, _, _), a, b) in enumerate(zip(NINE, got, base(variant))):
        if i != 3:
            same(a, b, name)


@pytest.mark.gpu
@pytest.mark.parametrize('fn,method', [('pipe_pr_cg_batch', 'pipe_pr_cg'), ('hs_cg_batch', 'hs_cg')])
def test_against_the_oracles_golden_histories(amd, matrices, fn, method):
    from test_gpu_parity import PREFIX_FLOOR
    names = ['bcsstk03', 'nos7']
    systems = [system(matrices, name) for name in names]
    max_iter = 40
    out = getattr(amd['cgv'], fn)([A for A, _ in systems], [b for _, b in systems], [np.zeros(b.size) for _, b in systems], max_iter,
                                  callbacks=[amd['cbs'].updated_residual_2_norm])
    assert len(out) == 2
    for name, trial in zip(names, out):
        ref = load_run(name, method, 'None')['hist_updated_residual_2_norm']
        prefix = PREFIX_FLOOR[name]
        assert trial['name'] == fn and trial['max_iter'] == max_iter and trial['updated_residual_2_norm'].shape == (max_iter,)
        np.testing.assert_allclose(trial['updated_residual_2_norm'][:prefix], ref[:prefix], rtol=1e-12, atol=0, err_msg=f'{name}/{fn}')


@pytest.mark.gpu
def test_refusals_through_the_c_abi(amd, matrices):
    L, P = amd['L'], amd['problems']
    lib = L.lib()
    A3, b3 = system(matrices, 'bcsstk03')
    A4 = system(matrices, 'nos4')[0]
    big = matrices['bcsstk14'][0]
    lap64 = P.laplace_2d(64, 64)
    op = amd['device'].DeviceCSR(A3)                 # an ordinary handle with an operator: left alone by every refusal
    h = op._h

    def create(mats, mat_of, handle=h, **edit):      # edit: name_ -> function applied to that argument
        rows_off, nnz_off, indptr, indices, data = csr_cat(mats)
        arg = dict(rows_off=rows_off, nnz_off=nnz_off, indptr=indptr, indices=indices, data=data,
                   mat_of=np.asarray(mat_of, dtype=np.int32), n_sys=len(mat_of), n_mat=len(mats))
        for key, fn in edit.items():
            arg[key[:-1]] = fn(arg[key[:-1]])
        out = C.c_void_p()
        rc = lib.prcg_batch_create(handle, arg['n_mat'], L.ptr(arg['rows_off']), L.ptr(arg['nnz_off']), L.ptr(arg['indptr']),
                                   L.ptr(arg['indices']), L.ptr(arg['data']), arg['n_sys'], L.ptr(arg['mat_of']), C.byref(out))
        return rc, out, (lib.prcg_last_error(handle) or b'').decode()

    def refused(text, *a, **k):
        rc, out, msg = create(*a, **k)
        assert rc == L.EINVAL and not out.value and re.search(text, msg), (rc, msg)

    def bump(i, by):
        def f(a):
            a = a.copy()
            a[i] += by
            return a
        return f
    try:
        refused(r'system 2 \(n = 1806, nnz = 63454', [A3, A4, big], [0, 1, 2])
        refused(r'system 1 \(n = 4096.*does not fit', [A3, lap64, big], [0, 1, 2])
        refused(r'system 3 ', [A3, lap64], [0, 0, 0, 1])
        refused(r'n_sys = 0', [A3], [])
        refused(r'mat_of\[1\] = 2 lies outside \[0, 2\)', [A3, A4], [0, 2, 1])
        refused(r'mat_of\[0\] = -1', [A3, A4], [-1, 0])
        refused(r'inconsistent offsets', [A3, A4], [0, 1], rows_off_=bump(0, 1))
        refused(r'inconsistent offsets: matrix 1 has 0 rows', [A3, A4], [0, 1], rows_off_=bump(2, -A4.shape[0]))
        refused(r'inconsistent offsets: indptr of matrix 1', [A3, A4], [0, 1], nnz_off_=bump(2, 1))
        refused(r'inconsistent offsets: indptr of matrix 0 decreases at row 3', [A3, A4], [0, 1], indptr_=bump(4, -10))
        refused(r'column index 100 of matrix 1 .* lies outside its 100 columns', [A3, A4], [0, 1], indices_=bump(A3.nnz + 7, 100 - int(A4.indices[7])))
        refused(r'column index -1 of matrix 0', [A3, A4], [0, 1], indices_=bump(0, -1 - int(A3.indices[0])))
        for key in ('rows_off', 'nnz_off', 'indptr', 'indices', 'data', 'mat_of'):
            refused(r'null pointer', [A3], [0], **{key + '_': lambda a: None})
        # begin: variant, history bit, null pointer, max_iter
        rc, bt, msg = create([A3, A4], [0, 1, 0])
        assert rc == L.OK and bt.value, msg
        try:
            n_all = 2 * A3.shape[0] + A4.shape[0]
            rhs, x0 = np.ones(n_all), np.zeros(n_all)

            def begin_refused(text, variant=L.PIPE_PR, r=rhs, x=x0, max_iter=5, mask=1):
                rc = lib.prcg_batch_begin(bt, variant, L.ptr(r), L.ptr(x), max_iter, mask)
                assert rc == L.EINVAL and re.search(text, lib.prcg_last_error(h).decode()), (rc, lib.prcg_last_error(h))
            for variant in (L.PIPE_P, L.PIPE_P_M, L.PR, L.M, L.CG_CG, L.GV, 99, -1):
                begin_refused(rf'variant {variant} is not served by a batch', variant=variant)
            for mask in (2, 4, 8, 3, 16):
                begin_refused(rf'history bits {mask}', mask=mask)
            begin_refused(r'null rhs or x0', r=None)
            begin_refused(r'null rhs or x0', x=None)
            begin_refused(r'max_iter = 0', max_iter=0)
            rc = lib.prcg_batch_iterate(bt, 1)
            assert rc == L.EINVAL and 'no open session' in lib.prcg_last_error(h).decode()
            # ... and a batch on a handle that holds an operator works, and leaves the operator alone
            assert lib.prcg_batch_begin(bt, L.HS, L.ptr(rhs), L.ptr(x0), 5, 1) == L.OK
            assert lib.prcg_batch_iterate(bt, 6) == L.EINVAL and 'exceed max_iter' in lib.prcg_last_error(h).decode()      # (as prcg_iterate: k + iters <= max_iter)
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
    with pytest.raises(L.PrcgError, match=r'system 1 \(n = 1806'):
        amd['device'].DeviceBatch([A3, big])


@pytest.mark.gpu
def test_refused_with_a_communicator(amd, matrices):
    """A communicator on the handle -- even of one rank -- and no batch is created on it."""
    from test_distributed import rccl_ids
    L = amd['L']
    A3 = system(matrices, 'bcsstk03')[0]
    rows_off, nnz_off, indptr, indices, data = csr_cat([A3])
    mat_of = np.zeros(1, dtype=np.int32)
    uid, path = rccl_ids(1)
    comm = amd['device'].DeviceCSR(A3, comm_init=(0, 1, uid, path))
    try:
        out = C.c_void_p()
        rc = L.lib().prcg_batch_create(comm._h, 1, L.ptr(rows_off), L.ptr(nnz_off), L.ptr(indptr), L.ptr(indices), L.ptr(data), 1,
                                       L.ptr(mat_of), C.byref(out))
        assert rc == L.EINVAL and not out.value and 'communicator' in L.lib().prcg_last_error(comm._h).decode()
    finally:
        comm.close()


@pytest.mark.gpu
def test_reference_shaped_functions(amd, matrices):
    L = amd['L']
    A, b = system(matrices, 'bcsstk03')
    n = A.shape[0]
    bs = [b, 2 * b, b + 1]
    out = amd['cgv'].pipe_pr_cg_batch(A, bs, [np.zeros(n)] * 3, 30, callbacks=[amd['cbs'].updated_residual_2_norm])
    assert len(out) == 3 and [t['name'] for t in out] == ['pipe_pr_cg_batch'] * 3 and [t['system'] for t in out] == [0, 1, 2]
    batch = amd['device'].DeviceBatch([A], [0, 0, 0])
    try:
        batch.begin(L.PIPE_PR, np.array(bs), np.zeros((3, n)), 30, hist_mask=1)
        batch.iterate(29)
        batch.sync()
        for s in range(3):
            assert np.array_equal(out[s]['updated_residual_2_norm'], batch.history(s)['updated_residual_2_norm'], equal_nan=True)
    finally:
        batch.close()
    # no recorder: no history, and the 2-D form of the vectors
    out = amd['cgv'].hs_cg_batch([A, A], np.array(bs[:2]), np.zeros((2, n)), 10)
    assert len(out) == 2 and 'updated_residual_2_norm' not in out[0]
