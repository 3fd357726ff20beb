"""Point-block Jacobi with VARIABLE block sizes, applied and built on the device (prcg.h: prcg_set_block_jacobi_var,
prcg_build_block_jacobi_var, prcg_get_block_jacobi_var; DeviceCSR.set_block_jacobi_var / build_block_jacobi_var /
get_block_jacobi_var; cg_variants.VarBlockJacobi, DeviceVarBlockJacobi; problems.fem_irregular_blocks).

The arithmetic is fixed by prcg.h -- the apply is one rounded product and one rounded sum per block entry in ascending column
order, the gather adds a row's entries in CSR order, the inversion is Gauss-Jordan without pivoting for exactly m_k steps -- so the
device kernels, the NumPy restatement and a plain loop must agree BIT FOR BIT, and on a uniform partition everything must carry
the bits of the uniform calls."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from new_cg_variants_amd import _lib as L
from new_cg_variants_amd import cg_variants as cgv
from new_cg_variants_amd import device, partition, problems
from new_cg_variants_amd.callbacks import updated_residual_2_norm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ITERS = 12
RAW_KNOBS = {'PRCG_WIN': '0', 'PRCG_SELL': '0'}      # a band as narrow as raw_operator's would get window tiles: keep the CSR-adaptive ones
BAD_TEXT = r'diagonal block {} \(size {}\) is singular or not finite'


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- partitions ---------------------------------------------------------------------------------------------------------
def from_sizes(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def mixed_partition(n, seed):
    """seeded sizes in 1..8, every size present (n >= 36), the last block trimmed to end at n"""
    rng = np.random.default_rng(seed)
    sizes = list(range(1, 9)) if n >= 36 else []
    while sum(sizes) < n:
        sizes.append(int(rng.integers(1, 9)))
    sizes[-1] -= sum(sizes) - n
    if sizes[-1] == 0:
        sizes.pop()
    order = rng.permutation(len(sizes))
    ptr = from_sizes([sizes[q] for q in order])
    assert ptr[-1] == n
    return ptr


def tile_count(ptr):
    """the greedy tiles of the device layout: consecutive whole blocks, at most 256 rows"""
    tiles, fill = 1, 0
    for m in np.diff(ptr):
        if fill + m > 256:
            tiles, fill = tiles + 1, 0
        fill += m
    return tiles


def uniform_partition(n, bs):
    return np.minimum(np.arange(0, n + bs, bs, dtype=np.int64), n)[:-(-n // bs) + 1]


@functools.lru_cache(maxsize=None)
def edge_partitions():
    """the smallest shapes at which the kernels can go wrong: (label, block_ptr)"""
    mix = from_sizes(np.random.default_rng(5).integers(1, 9, size=330))
    cases = [('one_row', from_sizes([1])), ('one_short_block', from_sizes([5])), ('600_ones', from_sizes([1] * 600)),
             ('560_eights', from_sizes([8] * 70)), ('255_threes_then_8', from_sizes([3] * 85 + [8])), ('mix', mix)]
    assert [tile_count(p) for _, p in cases] == [1, 1, 3, 3, 2, 6]
    assert set(np.diff(mix)) == set(range(1, 9)) and 1400 < mix[-1] < 1600
    return cases


EDGE_IDS = ['one_row', 'one_short_block', '600_ones', '560_eights', '255_threes_then_8', 'mix']


# ---- the contract, written out --------------------------------------------------------------------------------------------
def loop_apply(packed, ptr, v):
    out = np.zeros(v.shape[0])
    off = 0
    for k in range(len(ptr) - 1):
        r0, m = int(ptr[k]), int(ptr[k + 1] - ptr[k])
        for a in range(m):
            acc = packed[off + a * m] * v[r0]
            for j in range(1, m):
                acc = acc + packed[off + a * m + j] * v[r0 + j]
            out[r0 + a] = acc
        off += m * m
    return out


def loop_build(A, ptr):
    """gather in CSR order, Gauss-Jordan without pivoting for m steps, in NumPy doubles one operation at a time: packed"""
    out = []
    with np.errstate(all='ignore'):
        for k in range(len(ptr) - 1):
            r0, m = int(ptr[k]), int(ptr[k + 1] - ptr[k])
            M = [[np.float64(0.0)] * m for _ in range(m)]
            for a in range(m):
                for q in range(A.indptr[r0 + a], A.indptr[r0 + a + 1]):
                    c = int(A.indices[q])
                    if r0 <= c < r0 + m:
                        M[a][c - r0] = M[a][c - r0] + np.float64(A.data[q])
            E = [[np.float64(1.0 if r == j else 0.0) for j in range(m)] for r in range(m)]
            for c in range(m):
                p = M[c][c]
                M[c] = [M[c][j] / p for j in range(m)]
                E[c] = [E[c][j] / p for j in range(m)]
                for r in range(m):
                    if r != c:
                        f = M[r][c]
                        M[r] = [M[r][j] - f * M[c][j] for j in range(m)]
                        E[r] = [E[r][j] - f * E[c][j] for j in range(m)]
            out += [E[a][j] for a in range(m) for j in range(m)]
    return np.array(out, dtype=np.float64)


def packed_from_uniform(blocks, n):
    """(nb, bs, bs) of the uniform calls -> packed; the short last block as its leading part"""
    nb, bs = blocks.shape[:2]
    m = n - bs * (nb - 1)
    return np.concatenate([blocks[:nb - 1].reshape(-1), blocks[nb - 1, :m, :m].reshape(-1)])


# ---- operators ----------------------------------------------------------------------------------------------------------------
def dominant_spd(n, seed):
    """random sparse symmetric matrix with a strictly dominant positive diagonal"""
    rng = np.random.default_rng(seed)
    R = sp.random(n, n, density=min(1.0, 6.0 / max(n, 1)), random_state=rng, data_rvs=lambda k: rng.uniform(-1.0, 1.0, size=k))
    S = (R + R.T).tocsr()
    S = (S - sp.diags(S.diagonal())).tocsr()
    S.eliminate_zeros()
    d = np.asarray(abs(S).sum(axis=1)).ravel() + rng.uniform(1.0, 2.0, size=n)
    return (S + sp.diags(d)).tocsr()


@functools.lru_cache(maxsize=None)
def raw_operator():
    """The recipe of tests/test_block_jacobi_build.py::raw_operator: n = 511 from raw arrays, rows in random order with explicit
    duplicates, the diagonal stored as a triple whose sum depends on the order ((1e16, d, -1e16) or (1e16, -1e16, d), d in
    [4, 6)), off-diagonal values of size <= 0.05: strictly diagonally dominant."""
    rng = np.random.default_rng(17)
    n = 2 * 255 + 1
    indptr, indices, data = [0], [], []
    for i in range(n):
        k = int(rng.integers(1, 12))
        cols = list(np.clip(i + rng.integers(-12, 13, size=k), 0, n - 1))
        cols = [c for c in cols if c != i]
        cols += cols[:2]
        vals = list(rng.uniform(-0.05, 0.05, size=len(cols)))
        d = float(rng.uniform(4.0, 6.0))
        triple = [1e16, d, -1e16] if i % 3 == 0 else [1e16, -1e16, d]
        cols, vals = cols + [i, i, i], vals + triple
        order = rng.permutation(len(cols))
        pos = sorted(int(np.where(order == len(cols) - 3 + t)[0][0]) for t in range(3))
        for t in range(3):
            order[pos[t]] = len(cols) - 3 + t
        indices += [int(cols[j]) for j in order]
        data += [float(vals[j]) for j in order]
        indptr.append(len(indices))
    A = sp.csr_matrix((np.array(data), np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int32)), shape=(n, n))
    A.has_sorted_indices = False
    return A


@functools.lru_cache(maxsize=None)
def operator(name):
    if name == 'raw':
        return raw_operator()
    if name == 'irregular10':
        return problems.fem_irregular_3d(10).tocsr()
    if name == 's3_small':
        return problems.WORKLOADS['s3_small']['make']().tocsr()
    if name == 'lap3d':
        return problems.laplace_3d(21, 17, 13).tocsr()
    assert name == 'fem12'
    return problems.fem_like_3d(12).tocsr()


@functools.lru_cache(maxsize=None)
def partition_of(name):
    if name == 'irregular10':
        return problems.fem_irregular_blocks(10)
    return mixed_partition(operator(name).shape[0], seed=len(name))


@functools.lru_cache(maxsize=None)
def restatement(name):
    """the host restatement of the device build on a named operator and its partition, computed once"""
    return cgv.DeviceVarBlockJacobi(operator(name), partition_of(name)).inv_blocks


@functools.lru_cache(maxsize=None)
def edge_case(label):
    ptr = dict(edge_partitions())[label]
    A = dominant_spd(int(ptr[-1]), seed=int(ptr[-1]) % 97)
    return A, ptr, cgv.DeviceVarBlockJacobi(A, ptr)


def with_values(A, data):
    B = sp.csr_matrix((np.ascontiguousarray(data, dtype=np.float64), A.indices.copy(), A.indptr.copy()), shape=A.shape)
    B.has_sorted_indices = A.has_sorted_indices
    return B


def scaled(A, seed=3):
    """D A D with a seeded positive diagonal D"""
    d = np.random.default_rng(seed).uniform(0.5, 1.5, size=A.shape[0])
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    return with_values(A, d[rows] * A.data * d[A.indices[:A.nnz]])


@functools.lru_cache(maxsize=None)
def coupled_irregular():
    """fem_irregular_3d(10) plus strong intra-node coupling: Q diag(logspace(0, 3, m)) Q^T added to every node's diagonal block"""
    A, ptr = operator('irregular10'), problems.fem_irregular_blocks(10)
    rng = np.random.default_rng(0)
    rows, cols, vals = [], [], []
    for k in range(len(ptr) - 1):
        r0, m = int(ptr[k]), int(ptr[k + 1] - ptr[k])
        Q = np.linalg.qr(rng.standard_normal((m, m)))[0]
        B = Q @ np.diag(np.logspace(0, 3, m)) @ Q.T
        B = 0.5 * (B + B.T)
        ii, jj = np.meshgrid(np.arange(m), np.arange(m), indexing='ij')
        rows.append(r0 + ii.ravel()); cols.append(r0 + jj.ravel()); vals.append(B.ravel())
    n = A.shape[0]
    add = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    return (A + add).tocsr(), ptr


# ---------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, 'include', 'prcg.h')).read()
    assert 'int prcg_set_block_jacobi_var(prcg_t* h, int64_t nb, const int64_t* block_ptr, const double* inv_blocks);' in text
    assert 'int prcg_build_block_jacobi_var(prcg_t* h, int64_t nb, const int64_t* block_ptr, int64_t* first_bad_block);' in text
    assert 'int prcg_get_block_jacobi_var(prcg_t* h, double* inv_blocks);' in text
    assert '#define PRCG_SCHED_BLOCK_JACOBI_VAR 268435456' in text
    lib = L.lib()
    assert lib.prcg_version() == 1
    for name in ('prcg_set_block_jacobi_var', 'prcg_build_block_jacobi_var', 'prcg_get_block_jacobi_var'):
        assert hasattr(lib, name) and name in L._SIGNATURES
    ptr = from_sizes([2, 1])
    assert lib.prcg_set_block_jacobi_var(None, 2, L.ptr(ptr), None) == L.EINVAL
    assert lib.prcg_build_block_jacobi_var(None, 2, L.ptr(ptr), None) == L.EINVAL
    assert lib.prcg_get_block_jacobi_var(None, L.ptr(np.zeros(5))) == L.EINVAL
    for name in ('set_block_jacobi_var', 'build_block_jacobi_var', 'get_block_jacobi_var'):
        assert callable(getattr(device.DeviceCSR, name))
    assert 'VarBlockJacobi' in cgv.__all__ and 'DeviceVarBlockJacobi' in cgv.__all__


@pytest.mark.parametrize('cls', ['VarBlockJacobi', 'DeviceVarBlockJacobi'])
def test_the_callable_is_the_plain_loop(cls):
    ptr = mixed_partition(311, seed=2)
    assert set(np.diff(ptr)) == set(range(1, 9))
    A = dominant_spd(311, seed=8)
    P = getattr(cgv, cls)(A, ptr)
    assert P.n == 311 and np.array_equal(P.block_ptr, ptr) and P.inv_blocks.shape == (int((np.diff(ptr) ** 2).sum()),)
    v = np.random.default_rng(4).standard_normal(311)
    assert same_bits(P(v), loop_apply(P.inv_blocks, ptr, v))


def test_the_restatement_is_the_plain_loop():
    """the per-block gather in CSR order (unsorted rows, duplicates whose sum depends on the order) and invert_blocks per group of
    equal size, against one operation at a time"""
    A, ptr = operator('raw'), partition_of('raw')
    assert set(np.diff(ptr)) == set(range(1, 9))
    assert same_bits(restatement('raw'), loop_build(A, ptr))


@pytest.mark.parametrize('bs', [3, 5])
def test_uniform_partitions_carry_the_uniform_bits(bs):
    A = operator('fem12')
    n = A.shape[0]
    assert n == 5184
    ptr = uniform_partition(n, bs)
    assert ptr[-1] == n and (ptr[-1] - ptr[-2]) == (4 if bs == 5 else 3)
    U, P = cgv.DeviceBlockJacobi(A, bs), cgv.DeviceVarBlockJacobi(A, ptr)
    assert same_bits(P.inv_blocks, packed_from_uniform(U.inv_blocks, n))
    v = np.random.default_rng(bs).standard_normal(n)
    assert same_bits(P(v), U(v))


def test_lapack_inverses_on_nos7(matrices):
    A = matrices['nos7'][0].tocsr()
    ptr = mixed_partition(A.shape[0], seed=9)
    P = cgv.VarBlockJacobi(A, ptr)
    D = A.toarray()
    off = 0
    for k in range(len(ptr) - 1):
        r0, m = int(ptr[k]), int(ptr[k + 1] - ptr[k])
        B = P.inv_blocks[off:off + m * m].reshape(m, m)
        np.testing.assert_allclose(B @ D[r0:r0 + m, r0:r0 + m], np.eye(m), rtol=0, atol=1e-10)
        off += m * m


@pytest.mark.parametrize('cls', ['VarBlockJacobi', 'DeviceVarBlockJacobi'])
def test_constructors_refuse(cls):
    make = getattr(cgv, cls)
    A = dominant_spd(12, seed=1)
    with pytest.raises(ValueError, match=r'block_ptr\[0\] is 1, not 0'):
        make(A, [1, 4, 8, 12])
    with pytest.raises(ValueError, match=r'block_ptr\[nb\] is 11, not n_rows = 12'):
        make(A, [0, 4, 8, 11])
    with pytest.raises(ValueError, match='block 1 has size 0, outside 1..8'):
        make(A, [0, 4, 4, 12])
    with pytest.raises(ValueError, match='block 1 has size 9, outside 1..8'):
        make(A, [0, 1, 10, 12])
    D = A.toarray()
    D[5:8, :] = 0.0
    D[:, 5:8] = 0.0                                                   # block 2 of [0, 2, 5, 8, 12] is zero
    with pytest.raises(ValueError, match=cls + ': ' + BAD_TEXT.format(2, 3)):
        make(sp.csr_matrix(D), [0, 2, 5, 8, 12]).inv_blocks


@pytest.mark.parametrize('fn', ['hs_pcg_multi', 'pr_pcg_multi', 'pipe_pr_pcg_multi'])
def test_multi_rhs_functions_refuse_without_reading(fn):
    A = operator('irregular10')
    n = A.shape[0]
    P = cgv.DeviceVarBlockJacobi(A, problems.fem_irregular_blocks(10))
    B = np.ones((2, n))
    with pytest.raises(ValueError, match='block-Jacobi'):
        getattr(cgv, fn)(A, B, np.zeros((2, n)), 5, preconditioner=P)
    assert P._inv_blocks is None


def test_fem_irregular_blocks():
    ptr = problems.fem_irregular_blocks(10)
    assert ptr.dtype == np.int64 and ptr[0] == 0 and ptr[-1] == operator('irregular10').shape[0] == 3082
    assert np.bincount(np.diff(ptr), minlength=7).tolist() == [0, 277, 0, 511, 0, 0, 212]


def test_nodal_blocks_pay_where_the_coupling_is_nodal():
    """iterations of the oracle's hs_pcg until the updated residual falls below 1e-8 of its start: at most a tenth of Jacobi's"""
    from oracle import ne_oracle as orc
    A, ptr = coupled_irregular()
    n = A.shape[0]
    b, x0 = A @ (np.ones(n) / np.sqrt(n)), np.zeros(n)

    def count(P, max_iter):
        h = orc.hs_pcg(A, b, x0, max_iter, preconditioner=P, callbacks=['updated_residual_2_norm'])['updated_residual_2_norm']
        below = np.flatnonzero(h < 1e-8 * h[0])
        return int(below[0]) if below.size else max_iter
    nodal = count(cgv.DeviceVarBlockJacobi(A, ptr), 40)
    jacobi = count(cgv.Jacobi(A), 10 * nodal + 2)
    print(f'iterations to 1e-8: nodal blocks {nodal}, Jacobi {jacobi} (cap {10 * nodal + 2})')
    assert 10 * nodal <= jacobi


def test_host_layout_under_sanitizers(tmp_path):
    """the tiling / lay / unlay code of the library is host-only C++: a stand-alone program over the edge partitions, built with
    AddressSanitizer and UBSan, run on the CPU"""
    cxx = shutil.which('g++') or shutil.which('c++') or shutil.which('clang++')
    assert cxx, 'no host C++ compiler'
    exe = str(tmp_path / 'bjvar_layout_check')
    subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    '-I' + os.path.join(ROOT, 'new_cg_variants_amd', 'csrc'), os.path.join(ROOT, 'tests', 'host', 'bjvar_layout_check.cpp'),
                    '-o', exe], check=True, timeout=300)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and 'bjvar layout ok' in res.stdout, res.stdout[-2000:] + res.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('label', EDGE_IDS)
def test_bits_of_the_apply(label):
    """x0 = 0, so r_0 = b exactly: rt of a Hestenes-Stiefel session is M^-1 b (the single-vector kernel, unit stride); wt, ut of a
    pipelined session are M^-1 w, M^-1 u (the pair kernel)"""
    A, ptr, P = edge_case(label)
    n = A.shape[0]
    b, x0 = np.random.default_rng(n).standard_normal(n), np.zeros(n)
    op = device.DeviceCSR(A)
    try:
        op.begin(L.HS, b, x0, 3, block_jacobi_var=(ptr, P.inv_blocks))
        sched = op.schedule()
        assert sched['block_jacobi'] and sched['block_jacobi_var']
        assert same_bits(op.get_vector('r'), b)
        assert same_bits(op.get_vector('rt'), P(b))
        op.begin(L.PIPE_PR, b, x0, 3, block_jacobi_var=(ptr, P.inv_blocks))
        w, u = op.get_vector('w'), op.get_vector('u')
        assert np.any(w != 0.0) and np.any(u != 0.0)
        assert same_bits(op.get_vector('wt'), P(w))
        assert same_bits(op.get_vector('ut'), P(u))
        assert same_bits(op.get_vector('rt'), P(b))                   # (strided source and destination: a column of a pair array)
        op.iterate(2)
        op.sync()
        w, u = op.get_vector('w'), op.get_vector('u')
        assert same_bits(op.get_vector('wt'), P(w)) and same_bits(op.get_vector('ut'), P(u))
    finally:
        op.close()


def read_session(op):
    out = {'schedule': op.schedule()}
    for name in L.VEC:
        try:
            out[f'vector {name}'] = op.get_vector(name)
        except L.PrcgError:
            out[f'vector {name}'] = None
    for k in range(ITERS + 1):
        out[f'scalars {k}'] = op.get_scalars(k)
    for k in range(1, ITERS + 1):
        out[f'coefficients {k}'] = op.get_coefficients(k)
    for q, v in op.history().items():
        out[f'history {q}'] = v
    return out


def run_session(op, variant, b, x0, **kw):
    op.begin(variant, b, x0, ITERS + 1, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM | L.HIST_RESIDUAL_2_NORM, **kw)
    op.iterate(ITERS)
    assert op.k == ITERS
    return read_session(op)


@pytest.mark.gpu
@pytest.mark.parametrize('bs', [3, 5])
def test_uniform_partitions_run_the_uniform_sessions(bs):
    A = operator('fem12')
    n = A.shape[0]
    ptr = uniform_partition(n, bs)
    blocks = cgv.DeviceBlockJacobi(A, bs).inv_blocks
    packed = packed_from_uniform(blocks, n)
    rng = np.random.default_rng(21)
    b, x0 = rng.standard_normal(n), np.zeros(n)
    op, ref = device.DeviceCSR(A), device.DeviceCSR(A)
    try:
        for variant in (L.HS, L.PR, L.PIPE_PR, L.PIPE_P):
            got = run_session(op, variant, b, x0, block_jacobi_var=(ptr, packed))
            want = run_session(ref, variant, b, x0, block_jacobi=(bs, blocks))
            assert got['schedule']['block_jacobi'] and got['schedule']['block_jacobi_var']
            assert want['schedule']['block_jacobi'] and not want['schedule']['block_jacobi_var']
            assert got.keys() == want.keys()
            for key in got:
                if key == 'schedule':
                    assert {**got[key], 'block_jacobi_var': False} == want[key], variant
                elif got[key] is None or want[key] is None:
                    assert got[key] is None and want[key] is None, (variant, key)
                else:
                    assert same_bits(got[key], want[key]) and np.all(np.isfinite(got[key])), (variant, key)
            assert sum(v is not None for k, v in got.items() if k.startswith('vector')) >= 4
    finally:
        op.close()
        ref.close()


BUILD_CASES = [('irregular10', {}), ('raw', RAW_KNOBS), ('s3_small', {}), ('lap3d', {})]


@pytest.mark.gpu
@pytest.mark.parametrize('case', BUILD_CASES, ids=[c[0] for c in BUILD_CASES])
def test_bits_of_the_build(case):
    """irregular sliced rows with the nodal partition; the raw-array matrix (CSR-adaptive tiles, unsorted rows, duplicates whose sum
    depends on the order), s3_small with its value dictionary (the re-planned route) and lap3d (pattern tiles) with seeded mixes"""
    name, knobs = case
    A, ptr = operator(name), partition_of(name)
    op = device.DeviceCSR(A, knobs=knobs)
    try:
        sched = op.schedule()
        if name == 'irregular10':
            assert sched['sliced_rows']
        if name == 'raw':
            assert not sched['sliced_rows'] and not sched['window']
        if name == 's3_small':
            assert sched['value_dict'] and op.values_route() == 'replanned'
        if name == 'lap3d':
            assert sched['pattern']
        with pytest.raises(L.PrcgError, match='no block-Jacobi blocks'):
            op.get_block_jacobi_var(ptr)
        op.build_block_jacobi_var(ptr)
        assert same_bits(op.get_block_jacobi_var(), restatement(name)), name
    finally:
        op.close()


@pytest.mark.gpu
@pytest.mark.parametrize('label', EDGE_IDS)
def test_bits_of_the_build_at_tile_edges(label):
    A, ptr, P = edge_case(label)
    op = device.DeviceCSR(A)
    try:
        op.build_block_jacobi_var(ptr)
        assert same_bits(op.get_block_jacobi_var(), P.inv_blocks)
    finally:
        op.close()


@pytest.mark.gpu
def test_after_update_values():
    A, ptr = operator('irregular10'), partition_of('irregular10')
    B = scaled(A)
    want_new = cgv.DeviceVarBlockJacobi(B, ptr).inv_blocks
    op = device.DeviceCSR(A)
    try:
        op.build_block_jacobi_var(ptr)
        old = op.get_block_jacobi_var()
        assert same_bits(old, restatement('irregular10')) and np.array_equal(op._bjv_built, ptr)
        op.update_values(B.data)
        assert op._bjv_built is None and same_bits(op.get_block_jacobi_var(), old)          # frozen
        op.build_block_jacobi_var(ptr)
        new = op.get_block_jacobi_var()
        assert same_bits(new, want_new) and not same_bits(new, old)
    finally:
        op.close()


@pytest.mark.gpu
def test_round_trip():
    A, ptr, P = edge_case('mix')
    junk = np.random.default_rng(3).standard_normal(P.inv_blocks.shape)
    op = device.DeviceCSR(A)
    try:
        for blocks in (P.inv_blocks, junk):
            op.set_block_jacobi_var(ptr, blocks)
            assert same_bits(op.get_block_jacobi_var(), blocks)
        with pytest.raises(L.PrcgError, match='variable sizes: call prcg_get_block_jacobi_var'):
            op.get_block_jacobi(bs=3)
        op.set_block_jacobi(3, np.tile(np.eye(3), (-(-A.shape[0] // 3), 1, 1)))
        with pytest.raises(L.PrcgError, match='one uniform size: call prcg_get_block_jacobi'):
            op.get_block_jacobi_var(ptr)
        op.set_block_jacobi_var(ptr, junk)
        op.set_block_jacobi_var(None, None)
        with pytest.raises(L.PrcgError, match='no block-Jacobi blocks'):
            op.get_block_jacobi_var(ptr)
    finally:
        op.close()


@pytest.mark.gpu
def test_the_two_kinds_replace_each_other_in_sessions():
    """built blocks of one kind are not mistaken for blocks of the other: each session builds what it asks for, once"""
    A, ptr, P = edge_case('mix')
    n = A.shape[0]
    b, x0 = np.random.default_rng(2).standard_normal(n), np.zeros(n)
    uniform = cgv.DeviceBlockJacobi(A, 3)
    op = device.DeviceCSR(A)
    try:
        for _ in range(2):
            op.begin(L.HS, b, x0, 3, block_jacobi_var=(ptr, None))
            assert op.schedule()['block_jacobi_var'] and op._bj_built is None and np.array_equal(op._bjv_built, ptr)
            assert same_bits(op.get_vector('rt'), P(b)) and same_bits(op.get_block_jacobi_var(), P.inv_blocks)
            op.begin(L.HS, b, x0, 3, block_jacobi=(3, None))
            sched = op.schedule()
            assert sched['block_jacobi'] and not sched['block_jacobi_var'] and op._bj_built == 3 and op._bjv_built is None
            assert same_bits(op.get_vector('rt'), uniform(b)) and same_bits(op.get_block_jacobi(), uniform.inv_blocks)
        other = from_sizes([2] * (n // 2))                             # another partition of the same rows: built anew
        op.begin(L.HS, b, x0, 3, block_jacobi_var=(ptr, None))
        op.begin(L.HS, b, x0, 3, block_jacobi_var=(other, None))
        assert same_bits(op.get_block_jacobi_var(), cgv.DeviceVarBlockJacobi(A, other).inv_blocks)
        op.begin(L.HS, b, x0, 3)                                      # a plain session removes them
        assert not op.schedule()['block_jacobi'] and op._bjv_ptr is None
    finally:
        op.close()


@pytest.mark.gpu
def test_a_bad_block_is_reported_and_leaves_no_blocks():
    ptr = mixed_partition(200, seed=6)
    sizes = np.diff(ptr)
    K = int(np.flatnonzero(sizes >= 2)[3])                            # a block of at least two rows, with fine blocks before it
    K2 = int(np.flatnonzero(sizes >= 2)[7])
    D = dominant_spd(200, seed=5).toarray()
    for k in (K, K2):                                                 # the smallest index is reported
        D[ptr[k]:ptr[k + 1], ptr[k]:ptr[k + 1]] = 0.0
    A = sp.csr_matrix(D)
    n = 200
    b, x0 = np.random.default_rng(1).standard_normal(n), np.zeros(n)
    lib = L.lib()
    op = device.DeviceCSR(A)
    try:
        op.set_block_jacobi_var(ptr, np.ones(int((sizes ** 2).sum())))      # blocks set before are dropped by the failing build
        bad = C.c_int64(-5)
        assert lib.prcg_build_block_jacobi_var(op._h, len(ptr) - 1, L.ptr(ptr), C.byref(bad)) == L.EINVAL
        assert bad.value == K
        assert f'diagonal block {K} (size {sizes[K]}) is singular or not finite' in lib.prcg_last_error(op._h).decode()
        assert lib.prcg_get_block_jacobi_var(op._h, L.ptr(np.zeros(n * 8))) == L.EINVAL
        assert b'no block-Jacobi blocks' in lib.prcg_last_error(op._h)
        with pytest.raises(ValueError, match=BAD_TEXT.format(K, sizes[K])):
            op.build_block_jacobi_var(ptr)
        assert op._bjv_built is None and op._bjv_ptr is None
        with pytest.raises(ValueError, match='DeviceVarBlockJacobi: ' + BAD_TEXT.format(K, sizes[K])):
            cgv.DeviceVarBlockJacobi(A, ptr).inv_blocks               # the host restatement names the same block
        op.begin(L.HS, b, x0, 5)                                      # the next plain session runs
        op.iterate(4)
        op.sync()
        assert not op.schedule()['block_jacobi'] and not op.schedule()['block_jacobi_var']
    finally:
        op.close()


@pytest.mark.gpu
def test_refusals_leave_the_handle_as_it_was():
    lib = L.lib()
    h = C.c_void_p()
    assert lib.prcg_create(C.byref(h), 0) == L.OK
    try:
        p3 = from_sizes([3])
        assert lib.prcg_build_block_jacobi_var(h, 1, L.ptr(p3), None) == L.EINVAL and b'no operator' in lib.prcg_last_error(h)
        assert lib.prcg_set_block_jacobi_var(h, 1, L.ptr(p3), L.ptr(np.ones(9))) == L.EINVAL and b'no operator' in lib.prcg_last_error(h)
        assert lib.prcg_set_block_jacobi_var(h, 1, L.ptr(p3), None) == L.OK                   # removing nothing is fine
    finally:
        lib.prcg_destroy(h)
    A = operator('fem12')
    n = A.shape[0]
    x = np.random.default_rng(1).standard_normal(n)
    good = uniform_partition(n, 3)
    invalid = [(None, 'null block_ptr'),
               (good + 1, r'block_ptr\[0\] is 1, not 0'),
               (np.concatenate([good[:-1], [n + 1]]), rf'block_ptr\[nb\] is {n + 1}, not n_rows = {n}'),
               (np.concatenate([good[:7], good[7:8], good[7:]]), 'block 7 has size 0, outside 1..8'),
               (np.concatenate([good[:5], good[7:]]), 'block 4 has size 9, outside 1..8')]
    op = device.DeviceCSR(A)
    try:
        op.build_block_jacobi(3)
        before, y0 = op.get_block_jacobi(), op.matvec(x)[0]
        for ptr, text in invalid:
            nb = 3 if ptr is None else len(ptr) - 1
            pp = None if ptr is None else np.ascontiguousarray(ptr, dtype=np.int64)
            for rc in (lib.prcg_set_block_jacobi_var(op._h, nb, L.ptr(pp), L.ptr(np.ones(8 * n))),
                       lib.prcg_build_block_jacobi_var(op._h, nb, L.ptr(pp), None)):
                assert rc == L.EINVAL
            with pytest.raises(L.PrcgError, match=text):
                L.check(op._h, lib.prcg_build_block_jacobi_var(op._h, nb, L.ptr(pp), None))
            with pytest.raises(L.PrcgError, match=text):
                L.check(op._h, lib.prcg_set_block_jacobi_var(op._h, nb, L.ptr(pp), L.ptr(np.ones(8 * n))))
        assert op._bj_built == 3 and same_bits(op.get_block_jacobi(), before) and same_bits(op.matvec(x)[0], y0)
        assert lib.prcg_get_block_jacobi_var(op._h, L.ptr(np.zeros(8 * n))) == L.EINVAL
        # the multi-RHS sessions refuse variable blocks as they refuse uniform ones
        op.build_block_jacobi_var(good)
        B, X0 = np.ones((2, n)), np.zeros((2, n))
        with pytest.raises(L.PrcgError, match='prcg_solve_begin_multi: a block-Jacobi preconditioner is set'):
            op.begin_multi(L.HS, B, X0, 4)
        with pytest.raises(L.PrcgError, match='prcg_solve_begin_multi_pipe: a block-Jacobi preconditioner is set'):
            op.begin_multi_pipe(L.PIPE_PR, B, X0, 4)
        assert lib.prcg_get_block_jacobi_var(op._h, None) == L.EINVAL and b'null output' in lib.prcg_last_error(op._h)
    finally:
        op.close()
    # a row block with ghost columns: the build is refused
    blk, _ = partition.localize(problems.fem_like_3d(10)[900:2100], 900, 2100)
    blk = blk.tocsr()
    assert blk.shape[1] > blk.shape[0]
    x_ext = np.random.default_rng(2).standard_normal(blk.shape[1])
    op = device.DeviceCSR(blk)
    try:
        y0 = op.matvec_ext(x_ext)
        with pytest.raises(L.PrcgError, match='ghost columns') as err:
            op.build_block_jacobi_var(uniform_partition(blk.shape[0], 3))
        assert err.value.code == L.EINVAL and op._bjv_built is None
        assert same_bits(op.matvec_ext(x_ext), y0)
    finally:
        op.close()


@pytest.mark.gpu
def test_the_public_path_builds_on_the_device(monkeypatch):
    A = operator('irregular10').copy()
    ptr = partition_of('irregular10')
    n = A.shape[0]
    b, x0 = np.random.default_rng(21).standard_normal(n), np.zeros(n)
    builds = []
    real_build = device.DeviceCSR.build_block_jacobi_var
    monkeypatch.setattr(device.DeviceCSR, 'build_block_jacobi_var', lambda self, p: builds.append(1) or real_build(self, p))
    cgv.clear_operator_cache()
    fresh = device.DeviceCSR(A)
    try:
        P = cgv.DeviceVarBlockJacobi(A, ptr)
        out = cgv.pipe_pr_pcg(A, b, x0, 13, callbacks=[updated_residual_2_norm], preconditioner=P)
        assert P._inv_blocks is None and builds == [1]
        op = cgv._operator(A, 0)
        assert op.schedule()['block_jacobi_var'] and same_bits(op.get_block_jacobi_var(), restatement('irregular10'))
        fresh.begin(L.PIPE_PR, b, x0, 13, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM, block_jacobi_var=(ptr, restatement('irregular10')))
        fresh.iterate(12)
        fresh.sync()
        want = fresh.history()['updated_residual_2_norm']
        assert same_bits(out['updated_residual_2_norm'], want) and np.all(np.isfinite(want)) and want[12] < want[0]
        cgv.pipe_pr_pcg(A, b, x0, 13, callbacks=[updated_residual_2_norm], preconditioner=cgv.DeviceVarBlockJacobi(A, ptr))
        assert builds == [1]                                          # the blocks of that partition are in force: not built again
        A.data[:] = scaled(A).data
        assert cgv.update_values(A) == 'in_place'
        out2 = cgv.pipe_pr_pcg(A, b, x0, 13, callbacks=[updated_residual_2_norm], preconditioner=cgv.DeviceVarBlockJacobi(A, ptr))
        assert builds == [1, 1] and P._inv_blocks is None
        assert same_bits(cgv._operator(A, 0).get_block_jacobi_var(), cgv.DeviceVarBlockJacobi(A, ptr).inv_blocks)
        assert not same_bits(out2['updated_residual_2_norm'], out['updated_residual_2_norm'])
    finally:
        fresh.close()
        cgv.clear_operator_cache()
