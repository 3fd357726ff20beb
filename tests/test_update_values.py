"""New values on an unchanged sparsity pattern (prcg.h: prcg_update_values; DeviceCSR.update_values; cg_variants.update_values).

Route 0, in place: no encoding of the operator holds values -- the handle keeps its plan, the values are copied and, for sliced
rows, re-laid by k_sell_set_values.  Route 1, re-planned: a value dictionary or pattern tiles hold values -- plan and upload as
prcg_set_csr does.  Either way the handle must then compute, bit for bit, what a fresh handle on the new matrix computes; the CPU
tests establish that such a fresh handle runs the same plan (same tiles, slices, codes: the same summation order)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from new_cg_variants_amd import _lib as L
from new_cg_variants_amd import device, partition, problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 20


# ---- operators ----------------------------------------------------------------------------------------------------------
def ragged_operator():
    """the `ragged` operator of tests/test_abi_and_planning.py::test_sliced_row_layout_holds_exactly_the_matrix: rows of 40..50
    nonzeros, sixty of them empty, unsorted columns with duplicates"""
    rng = np.random.default_rng(9)
    n = 5000
    lens = rng.integers(40, 51, size=n)
    lens[rng.integers(0, n, size=60)] = 0
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    r = np.repeat(np.arange(n), lens)
    return sp.csr_matrix((rng.standard_normal(r.size), (r + rng.integers(-900, 901, size=r.size)).clip(0, n - 1).astype(np.int32), indptr),
                         shape=(n, n))


def gaps_operator():
    """Slices with skip positions on a square matrix: n = 110,000, 36 nonzeros per row in three clusters of 12 distinct ascending
    columns that start at i mod 4000, + 52,000 and + 104,000 (offsets inside a cluster below 400) -- the step from cluster to
    cluster is wider than one 16-bit delta code holds (49,150) --; in every 997th row entries 3 and 14 are exchanged (unsorted:
    a step forward and a step back by ~52,000)."""
    rng = np.random.default_rng(4)
    n = 110_000
    off = np.cumsum(rng.integers(1, 34, size=(n, 3, 12)), axis=2) - 1            # distinct, ascending, at most 12 * 33 - 1 = 395
    cols = (np.arange(n) % 4000)[:, None, None] + np.array([0, 52_000, 104_000])[None, :, None] + off
    cols = cols.reshape(n, 36)
    odd = np.arange(0, n, 997)
    cols[odd, 3], cols[odd, 14] = cols[odd, 14].copy(), cols[odd, 3].copy()
    assert cols.min() >= 0 and cols.max() < n
    A = sp.csr_matrix((rng.standard_normal(36 * n), cols.ravel().astype(np.int32), np.arange(n + 1, dtype=np.int32) * 36), shape=(n, n))
    A.has_sorted_indices = False
    return A


@functools.lru_cache(maxsize=None)
def operator(name):
    """The test operators, built once and never modified (the tests copy before they change values)."""
    if name == 'ragged':
        return ragged_operator()
    if name == 'gaps':
        return gaps_operator()
    if name == 's3_small':
        return problems.WORKLOADS['s3_small']['make']().tocsr()
    if name == 'lap3d':
        return problems.laplace_3d(21, 17, 13).tocsr()
    if name == 'irregular10':
        return problems.fem_irregular_3d(10).tocsr()
    if name == 'fem12_ones':
        A = problems.fem_like_3d(12).tocsr().copy()
        A.data[:] = 1.0
        return A
    assert name.startswith('fem')
    return problems.fem_like_3d(int(name[3:])).tocsr()


# (id, operator, knobs): what each pins is said in test_products_after_an_in_place_update
ROUTE0 = [
    ('fem11', 'fem11', {}),
    ('fem12_deltas', 'fem12', {'PRCG_SELL_WINDOW': '0'}),
    ('irregular', 'irregular10', {}),
    ('irregular_sigma256', 'irregular10', {'PRCG_SELL_SIGMA': '256'}),
    ('ragged', 'ragged', {}),
    ('fem12_csr', 'fem12', {'PRCG_SELL': '0'}),
    ('s3_plain', 's3_small', {'PRCG_VALDICT': '0'}),
    ('gaps', 'gaps', {}),
]
ROUTE0_GPU = ROUTE0 + [
    ('fem11_runs_off', 'fem11', {'PRCG_SELL_RUNS': '0'}),
    ('fem14_cut', 'fem14', {'PRCG_SELL_WINDOW': '24', 'PRCG_SELL_MAX_OVERHEAD_PCT': '600'}),
]
ROUTE1 = [
    ('s3_small', 's3_small', {}),
    ('lap3d', 'lap3d', {}),
    ('fem12_csr_ones', 'fem12_ones', {'PRCG_SELL': '0'}),
]


def with_values(A, data):
    """A's pattern -- the very index arrays' contents, order included -- with other values"""
    B = sp.csr_matrix((np.ascontiguousarray(data, dtype=np.float64), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    B.has_sorted_indices = A.has_sorted_indices
    return B


def scaled(A, seed=3):
    """D A D with a seeded random positive diagonal D: SPD stays SPD, and no value repeats"""
    d = np.random.default_rng(seed).uniform(0.5, 1.5, size=A.shape[0])
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return with_values(A, d[rows] * A.data * d[A.indices[:A.nnz]])


def wild_values(A, seed=7):
    """random values with +-0, +-inf and NaN sprinkled in"""
    rng = np.random.default_rng(seed)
    data = rng.standard_normal(A.nnz)
    for k, v in enumerate((0.0, -0.0, np.inf, -np.inf, np.nan)):
        data[rng.integers(0, A.nnz, size=max(3, A.nnz // 5000))] = v
    return with_values(A, data)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def same_bits_or_nan(a, b):
    """bit for bit, except that a NaN equals any NaN (the host and the device sign their default NaN differently)"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


# ---- CPU: declarations, routes, plan invariance ---------------------------------------------------------------------------
def test_entries_are_declared_and_bound():
    text = open(os.path.join(ROOT, 'include', 'prcg.h')).read()
    assert 'int prcg_update_values(prcg_t* h, const double* data, int data_on_device);' in text
    assert 'int prcg_values_route(const prcg_t* h);' in text
    assert 'int prcg_plan_values_route(' in open(os.path.join(ROOT, 'include', 'prcg_test.h')).read()
    lib = L.lib()
    for name in ('prcg_update_values', 'prcg_values_route', 'prcg_plan_values_route'):
        assert name in L._SIGNATURES and callable(getattr(lib, name))
    assert lib.prcg_values_route(None) == -1
    assert callable(device.DeviceCSR.update_values) and callable(device.DeviceCSR.values_route)
    from new_cg_variants_amd import cg_variants
    assert 'update_values' in cg_variants.__all__ and callable(cg_variants.update_values)


@pytest.mark.parametrize('case', ROUTE0, ids=[c[0] for c in ROUTE0])
def test_route_in_place_and_the_plan_does_not_depend_on_values(case):
    """No encoding holds values: route 0, and plan_operator of new values equals that of the old ones in every field except the
    two hashes that cover values (sliced rows hash the re-laid values as their dictionary) -- the in-place handle and a fresh
    handle on the new matrix run the same plan."""
    _, name, knobs = case
    A = operator(name)
    assert device.plan_values_route(A, knobs) == 'in_place'
    old = device.plan_operator(A, knobs)
    for B in (scaled(A), wild_values(A)):
        assert device.plan_values_route(B, knobs) == 'in_place'
        new = device.plan_operator(B, knobs)
        diff = {f for f in device.PLAN_OPERATOR_FIELDS if old[f] != new[f]}
        assert diff <= {'hash_dictionary', 'hash_value_index'}, diff
        assert not new['value_dict'] and not new['pattern']


@pytest.mark.parametrize('case', ROUTE1, ids=[c[0] for c in ROUTE1])
def test_route_replanned_where_an_encoding_holds_values(case):
    _, name, knobs = case
    A = operator(name)
    assert device.plan_values_route(A, knobs) == 'replanned'
    plan = device.plan_operator(A, knobs)
    assert plan['value_dict'] or plan['pattern']
    if name != 'fem12_ones':
        # values that never repeat: the dictionary falls to plain values, pattern tiles to index streams -- and the route to 0
        B = scaled(A)
        after = device.plan_operator(B, knobs)
        assert not after['value_dict'] and not after['pattern']
        assert device.plan_values_route(B, knobs) == 'in_place'


def test_gaps_operator_has_skip_positions():
    from test_abi_and_planning import plan_sell
    A = operator('gaps')
    n = A.shape[0]
    assert n == 110_000 and np.all(np.diff(A.indptr) == 36)
    got, slices, _, col, stats, rows = plan_sell(A)
    assert got > 0 and stats[10] == 0 and stats[9] == 1               # sliced rows, delta codes, a code per nonzero
    assert np.all(slices[:, 6] >= 0)                                 # every slice names its rows
    named = np.concatenate([rows[s[6]:s[6] + s[1] - s[0]] for s in slices])
    assert np.array_equal(np.sort(named[:, 0]), np.arange(n))
    skips = int(named[:, 1].sum()) - A.nnz                           # a skip code costs one stored position and names no nonzero
    assert skips > n, skips
    assert set(np.unique(named[:, 1]).tolist()) <= {38, 46} and 46 in named[:, 1]
    assert device.plan_operator(A)['family'] == 2


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def products(op, n, seed=11):
    """(matvec, matmat2, matmat4) of seeded random inputs"""
    rng = np.random.default_rng(seed)
    x, X2, X4 = rng.standard_normal(n), rng.standard_normal((n, 2)), rng.standard_normal((n, 4))
    return (x, op.matvec(x)[0]), (X2, op.matmat2(X2)[0]), (X4, op.matmat4(X4)[0])


def assert_products(op, fresh, B, label):
    """the three products of `op` equal scipy's per column and those of `fresh`"""
    got, want = products(op, B.shape[0]), products(fresh, B.shape[0])
    for (X, Y), (_, Yf) in zip(got, want):
        assert same_bits(Y, Yf), (label, 'against a fresh handle', Y.shape)
        cols = [(X, Y)] if X.ndim == 1 else [(X[:, j], Y[:, j]) for j in range(X.shape[1])]
        for j, (x, y) in enumerate(cols):
            assert same_bits_or_nan(y, B @ x), (label, 'against scipy', Y.shape, j)


@pytest.mark.gpu
@pytest.mark.parametrize('case', ROUTE0_GPU, ids=[c[0] for c in ROUTE0_GPU])
def test_products_after_an_in_place_update(case):
    """Each case pins one way k_sell_set_values can go wrong: fem11 (n = 3993) a ragged last slice; ragged empty rows and odd
    widths; irregular_sigma256 (and irregular) named rows; gaps skips; fem14_cut short slices in the middle of the table;
    fem11_runs_off against fem11 a code per nonzero against a code per run of three; fem12_csr and s3_plain the families whose
    kernels read the caller-order values.  The new values carry +-0, +-inf and NaN."""
    label, name, knobs = case
    A = operator(name)
    if label == 'fem14_cut':
        from test_abi_and_planning import plan_sell
        got, slices, _, _, stats, _ = plan_sell(A, sigma=64, window=24, max_overhead=6.0)
        assert got > 0 and stats[10] > 0 and np.count_nonzero(slices[:-1, 1] - slices[:-1, 0] < 64) > 10       # cut slices
    B = wild_values(A)
    op, fresh = device.DeviceCSR(A, knobs=knobs), device.DeviceCSR(B, knobs=knobs)
    try:
        before = (op.schedule(), op.layout(), op.operator_bytes())
        if label == 'fem14_cut':
            assert before[0]['sliced_rows'] and before[0]['window_codes']
        if label in ('irregular', 'irregular_sigma256'):
            assert before[0]['sorted_windows']
        assert op.values_route() == 'in_place'
        assert op.update_values(B.data) == 'in_place'
        after = (op.schedule(), op.layout(), op.operator_bytes())
        assert before[0] == after[0] and before[2] == after[2]
        assert before[1].keys() == after[1].keys() and all(np.array_equal(before[1][k], after[1][k]) for k in before[1])
        assert_products(op, fresh, B, label)
    finally:
        op.close()
        fresh.close()


CUDA_TENSOR_SCRIPT = r'''
import sys
import numpy as np
import torch                         # first: the library then binds to torch's HIP runtime, whose memory the tensors live in
sys.path.insert(0, sys.argv[1])
from new_cg_variants_amd import device, problems
A = problems.fem_like_3d(12).tocsr()
rng = np.random.default_rng(7)
data = rng.standard_normal(A.nnz)
data[::997] = -0.0; data[5::4001] = np.inf; data[9::5003] = np.nan
x = rng.standard_normal(A.shape[0])
host, dev = device.DeviceCSR(A), device.DeviceCSR(A)
assert host.update_values(data) == 'in_place'
t = torch.from_numpy(data).to('cuda:0')
assert dev.update_values(t) == 'in_place'
t.zero_()                            # the call has read the tensor: the caller may overwrite it
torch.cuda.synchronize()
yh, yd = host.matvec(x)[0], dev.matvec(x)[0]
assert np.array_equal(yh.view(np.uint64), yd.view(np.uint64)), 'device-tensor update differs from the host-array update'
assert dev.update_values(torch.from_numpy(data)) == 'in_place'          # a CPU tensor is an array
assert np.array_equal(yh.view(np.uint64), dev.matvec(x)[0].view(np.uint64))
big = torch.from_numpy(np.concatenate([data, data])).to('cuda:0')
for bad in (t.to(torch.float32), big[:A.nnz + 1], big[::2]):
    try:
        dev.update_values(bad)
    except ValueError:
        continue
    raise AssertionError('no ValueError for ' + str((bad.dtype, tuple(bad.shape), bad.is_contiguous())))
assert np.array_equal(yh.view(np.uint64), dev.matvec(x)[0].view(np.uint64))
print('cuda tensor ok')
'''


@pytest.mark.gpu
def test_update_from_a_cuda_tensor():
    """The device path: the values are read from a CUDA tensor where they lie; the result equals the host-array update bit for
    bit; float32, a wrong length and a non-contiguous view raise ValueError before the ABI is reached.  In a process of its
    own, which is what the test is about: a tensor's memory belongs to torch's HIP runtime, and the library reads it only when
    it is bound to that runtime -- torch imported before libprcg.so is loaded (as bench.py does)."""
    res = subprocess.run([sys.executable, '-c', CUDA_TENSOR_SCRIPT, ROOT], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and 'cuda tensor ok' in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


def read_session(op, multi=False):
    """everything a caller can read of the session `op` has run to iteration ITERS"""
    out = {'schedule': op.schedule()}
    for j in ((0, 1) if multi else (None,)):
        for name in L.VEC:
            try:
                out[f'vector {name} {j}'] = op.get_vector(name, rhs=j)
            except L.PrcgError:
                out[f'vector {name} {j}'] = None                       # not part of this session: on both handles or on neither
        for k in range(ITERS + 1):
            out[f'scalars {k} {j}'] = op.get_scalars(k, rhs=j)
        for k in range(1, ITERS + 1):
            out[f'coefficients {k} {j}'] = op.get_coefficients(k, rhs=j)
        for q, v in op.history(rhs=j).items():
            out[f'history {q} {j}'] = v
    return out


def run_session(op, variant, b, x0, inv_diag=None, multi=False, **kw):
    hist = L.HIST_UPDATED_RESIDUAL_2_NORM | (0 if multi else L.HIST_RESIDUAL_2_NORM)
    if multi:
        op.begin_multi_pipe(variant, b, x0, ITERS + 1, inv_diag=inv_diag, hist_mask=hist)
    else:
        op.begin(variant, b, x0, ITERS + 1, inv_diag=inv_diag, hist_mask=hist, **kw)
    op.iterate(ITERS)
    assert op.k == ITERS
    return read_session(op, multi)


def assert_same_session(label, got, want, finite=True):
    assert got.keys() == want.keys(), label
    for key in got:
        if key == 'schedule':
            assert got[key] == want[key], (label, {f: (got[key][f], want[key][f]) for f in got[key] if got[key][f] != want[key][f]})
        elif got[key] is None or want[key] is None:
            assert got[key] is None and want[key] is None, (label, key)
        else:
            assert same_bits(got[key], want[key]), (label, key)
            if finite:
                assert np.all(np.isfinite(got[key])), (label, key)
    assert sum(v is not None for k, v in got.items() if k.startswith('vector')) >= 4, label
    if finite:
        # the run did not break down: nu > 0 at every iteration, mu > 0 wherever an iteration followed
        for key in got:
            if key.startswith('scalars'):
                k = int(key.split()[1])
                assert got[key][L.S_NU] > 0 and (k == ITERS or got[key][L.S_MU] > 0), (label, key, got[key])


def rhs_for(n, seed=21):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n), np.zeros(n)


@pytest.mark.gpu
@pytest.mark.parametrize('case', [('fem12', 'fem12', {}), ('irregular', 'irregular10', {}), ('s3_plain', 's3_small', {'PRCG_VALDICT': '0'})],
                         ids=['fem12', 'irregular', 's3_plain'])
def test_sessions_after_an_in_place_update(case):
    """hs_pcg, pipe_pr_pcg and pr_pcg with Jacobi of the new diagonal on the updated handle: every vector, scalar row,
    coefficient and history is that of a fresh handle on the new matrix, bit for bit; on fem12 also a two-RHS pipelined session."""
    label, name, knobs = case
    A = operator(name)
    B = scaled(A)
    n = A.shape[0]
    b, x0 = rhs_for(n)
    inv_diag = 1.0 / B.diagonal()
    op, fresh = device.DeviceCSR(A, knobs=knobs), device.DeviceCSR(B, knobs=knobs)
    try:
        assert op.update_values(B.data) == 'in_place'
        for variant in ('HS', 'PIPE_PR', 'PR'):
            got = run_session(op, getattr(L, variant), b, x0, inv_diag)
            want = run_session(fresh, getattr(L, variant), b, x0, inv_diag)
            assert_same_session((label, variant), got, want)
        if label == 'fem12':
            b2, _ = rhs_for(n, seed=22)
            Bs, X0 = np.stack([b, b2]), np.zeros((2, n))
            got = run_session(op, L.PIPE_PR, Bs, X0, inv_diag, multi=True)
            want = run_session(fresh, L.PIPE_PR, Bs, X0, inv_diag, multi=True)
            assert got['schedule']['rhs2_pipe']
            assert_same_session((label, 'PIPE_PR x2'), got, want)
    finally:
        op.close()
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['s3_small', 'lap3d'])
def test_replanned_update_equals_a_fresh_handle(name):
    """Route 1: with the values x 1.5 the dictionary / the pattern tiles are kept, with D A D (values that never repeat) the
    dictionary falls to plain values and the pattern tiles to index streams; each time schedule, operator bytes, the products and
    a pipe_pr_cg session are those of a fresh handle."""
    A = operator(name)
    n = A.shape[0]
    b, x0 = rhs_for(n)
    kept = 'pattern' if name == 'lap3d' else 'value_dict'
    for step, B in (('x1.5', with_values(A, A.data * 1.5)), ('DAD', scaled(A))):
        op, fresh = device.DeviceCSR(A), device.DeviceCSR(B)
        try:
            assert op.schedule()[kept] and op.values_route() == 'replanned'
            assert op.update_values(B.data) == 'replanned'
            sched = op.schedule()
            assert sched == fresh.schedule() and op.operator_bytes() == fresh.operator_bytes(), (name, step)
            assert sched[kept] == (step == 'x1.5') and op.values_route() == ('replanned' if step == 'x1.5' else 'in_place')
            lay, layf = op.layout(), fresh.layout()
            assert all(np.array_equal(lay[k], layf[k]) for k in lay)
            assert_products(op, fresh, B, (name, step))
            got = run_session(op, L.PIPE_PR, b, x0)
            want = run_session(fresh, L.PIPE_PR, b, x0)
            assert_same_session((name, step), got, want)
            if step == 'DAD':
                # the in-place route does not decide again: the old values, which would qualify for the dictionary / the pattern
                # tiles, are served with plain values until the next prcg_set_csr -- and are served right
                assert op.update_values(A.data) == 'in_place' and not op.schedule()[kept]
                x = np.random.default_rng(5).standard_normal(n)
                assert same_bits(op.matvec(x)[0], A @ x)
        finally:
            op.close()
            fresh.close()


@pytest.mark.gpu
def test_preconditioner_and_options_stay_and_an_open_session_ends():
    from new_cg_variants_amd import cg_variants as cgv
    A = operator('fem12')
    B = scaled(A)
    n = A.shape[0]
    b, x0 = rhs_for(n)
    blocks = L.f64(cgv.BlockJacobi(A, 3).inv_blocks)                  # the OLD matrix's blocks: a frozen preconditioner
    hist = L.HIST_UPDATED_RESIDUAL_2_NORM | L.HIST_RESIDUAL_2_NORM
    op, fresh = device.DeviceCSR(A), device.DeviceCSR(B)
    lib = op._lib
    try:
        op._check(lib.prcg_set_block_jacobi(op._h, 3, L.ptr(blocks)))
        assert op.update_values(B.data) == 'in_place'
        # (DeviceCSR.begin sets or removes the blocks itself: the ABI call shows what the handle kept)
        op._check(lib.prcg_solve_begin(op._h, L.PIPE_PR, L.ptr(b), L.ptr(x0), ITERS + 1, None, None, hist))
        op.max_iter, op.hist_mask = ITERS + 1, hist
        assert op.schedule()['block_jacobi']
        op.iterate(ITERS)
        got = read_session(op)
        want = run_session(fresh, L.PIPE_PR, b, x0, block_jacobi=(3, blocks))
        assert want['schedule']['block_jacobi']
        assert_same_session('frozen block Jacobi', got, want)
        # an update in the middle of an open session ends it
        op.begin(L.HS, b, x0, ITERS + 1, inv_diag=1.0 / B.diagonal(), hist_mask=hist)
        op.iterate(3)
        assert op.update_values(B.data) == 'in_place'
        with pytest.raises(L.PrcgError, match='no open session') as err:
            op.iterate(1)
        assert err.value.code == L.EINVAL
        got = run_session(op, L.HS, b, x0, 1.0 / B.diagonal())
        want = run_session(fresh, L.HS, b, x0, 1.0 / B.diagonal())
        assert_same_session('after the interrupted session', got, want)
    finally:
        op.close()
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['fem12', 's3_small'])
def test_there_and_back_and_twice(name):
    """Update to other values and back: products and a session are what they were before the first update; two updates in a row
    behave as one.  s3_small goes to values x 1.5, which keep its dictionary (route 1 both ways); after D A D it would hold plain
    values and keep them (test_replanned_update_equals_a_fresh_handle)."""
    A = operator(name)
    B = scaled(A) if name == 'fem12' else with_values(A, A.data * 1.5)
    n = A.shape[0]
    b, x0 = rhs_for(n)
    route = 'in_place' if name == 'fem12' else 'replanned'
    op, fresh = device.DeviceCSR(A), device.DeviceCSR(B)
    try:
        prod0 = products(op, n)
        sess0 = run_session(op, L.PIPE_PR, b, x0)
        assert op.update_values(B.data) == route
        op.update_values(B.data)                                      # twice in a row: as once
        assert_products(op, fresh, B, (name, 'twice'))
        assert_same_session((name, 'twice'), run_session(op, L.PIPE_PR, b, x0), run_session(fresh, L.PIPE_PR, b, x0))
        op.update_values(A.data)                                      # and back
        assert op.values_route() == route
        for (_, y0), (_, y1) in zip(prod0, products(op, n)):
            assert same_bits(y0, y1), name
        assert_same_session((name, 'back'), run_session(op, L.PIPE_PR, b, x0), sess0)
    finally:
        op.close()
        fresh.close()


@pytest.mark.gpu
def test_refusals_leave_the_handle_as_it_was():
    lib = L.lib()
    some = np.ones(8)
    # before prcg_set_csr
    h = C.c_void_p()
    assert lib.prcg_create(C.byref(h), 0) == L.OK
    try:
        assert lib.prcg_values_route(h) == -1
        assert lib.prcg_update_values(h, L.ptr(some), 0) == L.EINVAL
        assert b'no operator' in lib.prcg_last_error(h)
    finally:
        lib.prcg_destroy(h)
    # null data, a data_on_device that is neither 0 nor 1 (checked before any pointer is looked at)
    A = operator('fem12')
    x = np.random.default_rng(1).standard_normal(A.shape[0])
    op = device.DeviceCSR(A)
    try:
        y0 = op.matvec(x)[0]
        assert lib.prcg_update_values(op._h, None, 0) == L.EINVAL and b'null data' in lib.prcg_last_error(op._h)
        assert lib.prcg_update_values(op._h, None, 1) == L.EINVAL and b'null data' in lib.prcg_last_error(op._h)
        assert lib.prcg_update_values(op._h, L.ptr(np.ones(A.nnz)), 2) == L.EINVAL and b'data_on_device' in lib.prcg_last_error(op._h)
        with pytest.raises(ValueError, match='nonzeros'):
            op.update_values(np.ones(A.nnz + 1))
        with pytest.raises(ValueError, match='fp64'):
            op.update_values(np.ones(A.nnz, dtype=np.float32))
        assert same_bits(op.matvec(x)[0], y0) and same_bits(y0, A @ x)
    finally:
        op.close()
    # a row block with ghost columns
    blk, _ = partition.localize(problems.fem_like_3d(10)[900:2100], 900, 2100)
    blk = blk.tocsr()
    assert blk.shape[1] > blk.shape[0]
    x_ext = np.random.default_rng(2).standard_normal(blk.shape[1])
    op = device.DeviceCSR(blk)
    try:
        y0 = op.matvec_ext(x_ext)
        with pytest.raises(L.PrcgError, match='ghost columns') as err:
            op.update_values(blk.data * 2.0)
        assert err.value.code == L.EINVAL
        assert same_bits(op.matvec_ext(x_ext), y0)
    finally:
        op.close()
    # a world size > 1 on the handle
    op = device.DeviceCSR(A, world=(0, 2))
    try:
        y0 = op.matvec(x)[0]
        with pytest.raises(L.PrcgError, match='world size') as err:
            op.update_values(A.data * 2.0)
        assert err.value.code == L.EINVAL
        assert same_bits(op.matvec(x)[0], y0) and same_bits(y0, A @ x)
    finally:
        op.close()


@pytest.mark.gpu
def test_cg_variants_update_values():
    from new_cg_variants_amd import cg_variants as cgv
    from new_cg_variants_amd.callbacks import updated_residual_2_norm
    A = operator('fem12').copy()
    n = A.shape[0]
    b, x0 = rhs_for(n)
    cgv.clear_operator_cache()
    try:
        assert cgv.update_values(A) is None                           # never solved with: nothing cached
        cgv.hs_pcg(A, b, x0, ITERS + 1, callbacks=[updated_residual_2_norm], preconditioner=lambda v: (1 / A.diagonal()) * v)
        cached = cgv._operator(A, 0)
        A.data[:] = scaled(A).data                                    # in place: the same arrays, new coefficients
        assert cgv.update_values(A) == 'in_place'
        assert len(cgv._OPERATORS) == 1 and cgv._operator(A, 0) is cached
        got = cgv.hs_pcg(A, b, x0, ITERS + 1, callbacks=[updated_residual_2_norm], preconditioner=lambda v: (1 / A.diagonal()) * v)
        assert len(cgv._OPERATORS) == 1
        cgv.clear_operator_cache()
        want = cgv.hs_pcg(A, b, x0, ITERS + 1, callbacks=[updated_residual_2_norm], preconditioner=lambda v: (1 / A.diagonal()) * v)
        assert same_bits(got['updated_residual_2_norm'], want['updated_residual_2_norm'])
        assert np.all(np.isfinite(got['updated_residual_2_norm']))
        assert cgv.update_values(operator('fem11')) is None
    finally:
        cgv.clear_operator_cache()
