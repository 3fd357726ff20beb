"""The block-Jacobi inverses built on the device from the operator (prcg.h: prcg_build_block_jacobi, prcg_get_block_jacobi;
DeviceCSR.build_block_jacobi / get_block_jacobi; cg_variants.invert_blocks, cg_variants.DeviceBlockJacobi).

The arithmetic is fixed by prcg.h -- the gather adds a row's entries in CSR order, the inversion is Gauss-Jordan without pivoting
with a division per pivot-row entry -- so the device kernel, `invert_blocks` (NumPy, vectorised over blocks) and a plain triple
loop must agree BIT FOR BIT on every block that is not bad, and a session whose blocks were built on the device must reproduce,
entry by entry, the session that was handed the same inverses through prcg_set_block_jacobi."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp

from new_cg_variants_amd import _lib as L
from new_cg_variants_amd import cg_variants as cgv
from new_cg_variants_amd import device, partition, problems
from test_update_values import ITERS, assert_same_session, operator, read_session, rhs_for, run_session, same_bits, scaled, with_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_NAMES = ['494_bus', 'bcsstk03', 'bcsstk14', 'bcsstm22', 'model_48_8_3', 'nos4', 'nos7']
RAW_KNOBS = {'PRCG_WIN': '0', 'PRCG_SELL': '0'}      # a band as narrow as raw_operator's would get window tiles: keep the CSR-adaptive ones
BAD_TEXT = r'diagonal block {} \(bs = {}\) is singular or not finite'


# ---- the contract, written out ------------------------------------------------------------------------------------------
def loop_apply(inv_blocks, bs, v):
    """The apply contract of prcg.h: blocks, rows, columns."""
    n = v.shape[0]
    out = np.zeros(n)
    for k in range(-(-n // bs)):
        cols = min(bs, n - k * bs)
        for a in range(cols):
            acc = inv_blocks[k, a, 0] * v[k * bs]
            for j in range(1, cols):
                acc = acc + inv_blocks[k, a, j] * v[k * bs + j]
            out[k * bs + a] = acc
    return out


def loop_invert(block):
    """The invert contract of prcg.h for ONE block, in Python floats (IEEE doubles, every operation rounded): (E, bad)."""
    bs = len(block)
    M = [[float(block[r][j]) for j in range(bs)] for r in range(bs)]
    E = [[1.0 if r == j else 0.0 for j in range(bs)] for r in range(bs)]
    bad = False
    for c in range(bs):
        p = M[c][c]
        bad = bad or p == 0.0 or not np.isfinite(p)
        with np.errstate(all='ignore'):
            M[c] = [float(np.float64(M[c][j]) / np.float64(p)) for j in range(bs)]
            E[c] = [float(np.float64(E[c][j]) / np.float64(p)) for j in range(bs)]
        for r in range(bs):
            if r == c:
                continue
            f = M[r][c]
            for j in range(bs):
                M[r][j] = M[r][j] - f * M[c][j]
                E[r][j] = E[r][j] - f * E[c][j]
    E = np.array(E)
    return E, bad or not np.isfinite(E).all()


def loop_gather(A, bs):
    """The gather contract of prcg.h, row by row in CSR order; a short last block inside an identity."""
    n = A.shape[0]
    nb = -(-n // bs)
    blocks = np.zeros((nb, bs, bs))
    for i in range(n):
        k, a = divmod(i, bs)
        for q in range(A.indptr[i], A.indptr[i + 1]):
            if A.indices[q] // bs == k:
                blocks[k, a, A.indices[q] % bs] = blocks[k, a, A.indices[q] % bs] + A.data[q]
    for i in range(n, nb * bs):
        blocks[nb - 1, i % bs, i % bs] = 1.0
    return blocks


def gathered(A, bs):
    """BlockJacobi._gather plus the identity around a short last block: what invert_blocks takes"""
    n = A.shape[0]
    nb = -(-n // bs)
    blocks = cgv.BlockJacobi._gather(A, n, nb, bs)
    m = n - bs * (nb - 1)
    if m < bs and nb > 0:
        blocks[-1, np.arange(m, bs), np.arange(m, bs)] = 1.0
    return blocks


@functools.lru_cache(maxsize=None)
def restatement(name, bs, which='old'):
    """invert_blocks(_gather(A)) of a named operator, computed once: the bits the device must produce"""
    A = named_operator(name)
    if which == 'new':
        A = new_values(name)
    inv, bad = cgv.invert_blocks(gathered(A, bs))
    assert not bad.any(), (name, bs, int(np.argmax(bad)))
    return inv


# ---- operators ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def raw_operator():
    """n = 2 * 255 + 1 (two whole tiles and one row at bs = 3), built from raw arrays: rows of 4..14 entries in random order, columns
    within +-12 of the diagonal with explicit duplicates, values of size <= 0.05 -- and the diagonal entry stored as a triple
    whose sum depends on the order, (1e16, d, -1e16) in every third row and (1e16, -1e16, d) elsewhere, d in [4, 6): strictly
    diagonally dominant, so no pivot of any diagonal block vanishes."""
    rng = np.random.default_rng(17)
    n = 2 * 255 + 1
    indptr, indices, data = [0], [], []
    for i in range(n):
        k = int(rng.integers(1, 12))
        cols = list(np.clip(i + rng.integers(-12, 13, size=k), 0, n - 1))
        cols = [c for c in cols if c != i]
        cols += cols[:2]                                           # explicit duplicates of off-diagonal entries
        vals = list(rng.uniform(-0.05, 0.05, size=len(cols)))
        d = float(rng.uniform(4.0, 6.0))
        triple = [1e16, d, -1e16] if i % 3 == 0 else [1e16, -1e16, d]
        cols, vals = cols + [i, i, i], vals + triple
        order = rng.permutation(len(cols))
        # the permutation keeps the triple's relative order (its sum is what the order decides): sort its three positions back
        pos = sorted(int(np.where(order == len(cols) - 3 + t)[0][0]) for t in range(3))
        for t in range(3):
            order[pos[t]] = len(cols) - 3 + t
        indices += [int(cols[j]) for j in order]
        data += [float(vals[j]) for j in order]
        indptr.append(len(indices))
    A = sp.csr_matrix((np.array(data), np.array(indices, dtype=np.int32), np.array(indptr, dtype=np.int32)), shape=(n, n))
    A.has_sorted_indices = False
    return A


def named_operator(name):
    if name == 'raw':
        return raw_operator()
    return operator({'s3_plain': 's3_small'}.get(name, name))


@functools.lru_cache(maxsize=None)
def new_values(name):
    """other values on the pattern of a named operator: D A D on fem12 (in place), x 1.5 on s3_small (keeps its dictionary)"""
    A = named_operator(name)
    return scaled(A) if name == 'fem12' else with_values(A, A.data * 1.5)


def dominant_spd(n, seed):
    """random sparse symmetric matrix with a strictly dominant positive diagonal"""
    rng = np.random.default_rng(seed)
    R = sp.random(n, n, density=min(1.0, 6.0 / max(n, 1)), random_state=rng, data_rvs=lambda k: rng.uniform(-1.0, 1.0, size=k))
    S = (R + R.T).tocsr()
    S = (S - sp.diags(S.diagonal())).tocsr()
    S.eliminate_zeros()
    d = np.asarray(abs(S).sum(axis=1)).ravel() + rng.uniform(1.0, 2.0, size=n)
    return (S + sp.diags(d)).tocsr()


def singular_example():
    """the matrix of tests/test_block_jacobi.py::test_singular_block_is_refused"""
    D = np.diag([2.0, 3.0, 4.0, 1.0, 0.0, 0.0, 6.0])
    D[0, 1] = D[1, 0] = 1.0
    D[3, 4] = D[4, 3] = 0.5
    return D


# ---------------------------------------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, 'include', 'prcg.h')).read()
    assert 'int prcg_build_block_jacobi(prcg_t* h, int bs, int64_t* first_bad_block);' in text
    assert 'int prcg_get_block_jacobi(prcg_t* h, double* inv_blocks);' in text
    lib = L.lib()
    for name in ('prcg_build_block_jacobi', 'prcg_get_block_jacobi'):
        assert name in L._SIGNATURES and callable(getattr(lib, name))
    bad = C.c_int64(7)
    assert lib.prcg_build_block_jacobi(None, 3, C.byref(bad)) == L.EINVAL
    assert lib.prcg_get_block_jacobi(None, L.ptr(np.zeros(9))) == L.EINVAL
    assert lib.prcg_version() == 1
    assert callable(device.DeviceCSR.build_block_jacobi) and callable(device.DeviceCSR.get_block_jacobi)
    assert 'invert_blocks' in cgv.__all__ and 'DeviceBlockJacobi' in cgv.__all__


@pytest.mark.parametrize('bs', range(1, 9))
def test_invert_blocks_is_the_plain_loop(bs):
    rng = np.random.default_rng(100 + bs)
    G = rng.standard_normal((40, bs, bs))
    blocks = G @ G.transpose(0, 2, 1) + 0.1 * np.eye(bs)             # random SPD blocks
    blocks[3] *= 1e-200
    blocks[4] *= 1e150
    inv, bad = cgv.invert_blocks(blocks)
    assert inv.shape == blocks.shape and bad.shape == (40,) and not bad.any()
    for k in range(40):
        want, wbad = loop_invert(blocks[k])
        assert not wbad
        assert same_bits(inv[k], want), (bs, k)
    np.testing.assert_allclose(inv[7] @ blocks[7], np.eye(bs), atol=1e-8)


def test_invert_blocks_flags_what_the_plain_loop_flags():
    blocks = np.array([[[2.0, 1.0], [1.0, 3.0]], [[0.0, 1.0], [1.0, 0.0]], [[1.0, 1.0], [1.0, 1.0]], [[np.nan, 0.0], [0.0, 1.0]],
                       [[np.inf, 0.0], [0.0, 1.0]], [[-0.0, 0.0], [0.0, 1.0]], [[4.0, -0.0], [-0.0, 2.0]]])
    inv, bad = cgv.invert_blocks(blocks)
    assert bad.tolist() == [False, True, True, True, True, True, False]
    for k in range(len(blocks)):
        want, wbad = loop_invert(blocks[k])
        assert wbad == bad[k], k
        if not wbad:
            assert same_bits(inv[k], want), k                        # signed zeros included
    assert same_bits(blocks, np.array(blocks))                        # the input is not modified


@pytest.mark.parametrize('bs', [2, 3, 6, 8])
@pytest.mark.parametrize('name', GOLDEN_NAMES)
def test_invert_blocks_against_lapack(matrices, name, bs):
    """max |inv - ref| / max |ref| per block <= 1e-10 on the gathered blocks of every golden matrix (2.8e-13 at worst, bcsstk14:
    block condition numbers up to 8e9; the margin covers another LAPACK build); no block is bad."""
    A, _ = matrices[name]
    blocks = gathered(A, bs)
    inv, bad = cgv.invert_blocks(blocks)
    assert not bad.any()
    ref = np.linalg.inv(blocks)
    err = np.abs(inv - ref).max(axis=(1, 2)) / np.abs(ref).max(axis=(1, 2))
    print(f'{name} bs={bs}: worst block error against LAPACK {err.max():.2e}')
    assert err.max() <= 1e-10, (name, bs, int(np.argmax(err)), err.max())


@pytest.mark.parametrize('bs', [1, 2, 3, 4, 7, 8])
@pytest.mark.parametrize('name', ['bcsstk03', 'nos7'])
def test_device_block_jacobi_as_a_callable(matrices, name, bs):
    A, _ = matrices[name]
    n = A.shape[0]
    P = cgv.DeviceBlockJacobi(A, bs)
    assert P._inv_blocks is None                                     # built on first use only
    nb = -(-n // bs)
    assert P.bs == bs and P.n == n and P.inv_blocks.shape == (nb, bs, bs)
    assert same_bits(P.inv_blocks, cgv.invert_blocks(gathered(A, bs))[0])
    m = n - bs * (nb - 1)
    if m < bs:
        pad = P.inv_blocks[-1].copy()
        pad[:m, :m] = np.eye(bs)[:m, :m]
        np.testing.assert_array_equal(pad, np.eye(bs))
    rng = np.random.default_rng(5)
    for v in (rng.standard_normal(n), np.ones(n), -rng.random(n) * 1e-300):
        assert same_bits(P(v), loop_apply(P.inv_blocks, bs, v))


@pytest.mark.parametrize('name', ['nos7', 'model_48_8_3'])
def test_the_blocks_are_the_inverses(matrices, name):
    A, _ = matrices[name]
    n = A.shape[0]
    for bs in (2, 3, 4, 7):
        P = cgv.DeviceBlockJacobi(A, bs)
        blocks = gathered(A, bs)
        prod = P.inv_blocks @ blocks
        assert np.abs(prod - np.eye(bs)).max() <= 1e-9, (name, bs)
    D = A.toarray()
    assert same_bits(gathered(A, 3)[1], D[3:6, 3:6]) and n > 6


def test_refusals_on_the_host_path():
    D = singular_example()
    A = sp.csr_matrix(D)
    with pytest.raises(ValueError, match='DeviceBlockJacobi: ' + BAD_TEXT.format(2, 2)):
        cgv.DeviceBlockJacobi(A, 2).inv_blocks
    with pytest.raises(ValueError, match=BAD_TEXT.format(4, 1)):
        cgv.DeviceBlockJacobi(A, 1)(np.ones(7))                      # the first zero on the diagonal
    with pytest.raises(ValueError, match='outside 1..8'):
        cgv.DeviceBlockJacobi(A, 9)
    with pytest.raises(ValueError, match='outside 1..8'):
        cgv.DeviceBlockJacobi(A, 0)
    D[0, 0] = np.nan
    with pytest.raises(ValueError, match=BAD_TEXT.format(0, 3)):
        cgv.DeviceBlockJacobi(sp.csr_matrix(D), 3).inv_blocks
    swap = sp.csr_matrix(np.array([[0.0, 1.0], [1.0, 0.0]]))
    np.testing.assert_array_equal(cgv.BlockJacobi(swap, 2).inv_blocks[0], [[0.0, 1.0], [1.0, 0.0]])      # LAPACK pivots
    with pytest.raises(ValueError, match=BAD_TEXT.format(0, 2)):
        cgv.DeviceBlockJacobi(swap, 2).inv_blocks


def test_multi_rhs_refuses_the_object_without_reading_it():
    A = operator('fem11')
    n = A.shape[0]
    P = cgv.DeviceBlockJacobi(A, 3)
    with pytest.raises(ValueError, match='block-Jacobi preconditioner is not served by the two-RHS session'):
        cgv.hs_pcg_multi(A, np.ones((2, n)), np.zeros((2, n)), 5, preconditioner=P)
    assert P._inv_blocks is None


@pytest.mark.parametrize('bs', [1, 2, 3, 5, 8])
def test_gather_adds_duplicates_in_csr_order(bs):
    A = raw_operator()
    n = A.shape[0]
    assert n == 2 * 255 + 1 and not A.has_sorted_indices
    # unsorted rows, explicit duplicates, and diagonal triples whose sum depends on the order
    row = slice(A.indptr[3], A.indptr[4])
    assert np.any(np.diff(A.indices[row]) < 0) and len(set(A.indices[row])) < A.indptr[4] - A.indptr[3]
    diag = np.array([[A.data[q] for q in range(A.indptr[i], A.indptr[i + 1]) if A.indices[q] == i] for i in (3, 4)])
    assert diag[0].tolist()[::2] == [1e16, -1e16] and diag[1].tolist()[:2] == [1e16, -1e16]
    want = loop_gather(A, bs)
    got = gathered(A, bs)
    assert same_bits(got, want)
    # row 4 sums to its d exactly, row 3 to d rounded to the spacing of doubles at 1e16
    assert want[4 // bs, 4 % bs, 4 % bs] == diag[1, 2] and want[3 // bs, 3 % bs, 3 % bs] in (4.0, 6.0)
    assert not cgv.invert_blocks(got)[1].any()
    assert device.plan_operator(A, RAW_KNOBS)['family'] == 0         # CSR-adaptive tiles


# ---------------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------------
BUILD_CASES = [('fem12', {}), ('irregular10', {}), ('s3_small', {}), ('s3_plain', {'PRCG_VALDICT': '0'}), ('lap3d', {}), ('raw', RAW_KNOBS)]


@pytest.mark.gpu
@pytest.mark.parametrize('case', BUILD_CASES, ids=[c[0] for c in BUILD_CASES])
def test_bits_of_the_build(case):
    """One operator per family: fem12 (n = 5184: sliced rows with window codes; 20 tiles of 255 rows plus a remainder at bs = 3, a
    short last block at bs = 5, 7), irregular10 (irregular sliced rows), s3_small with its value dictionary (the re-planning route
    of update_values) and with plain values, lap3d (pattern tiles), the raw-array matrix (CSR-adaptive tiles, unsorted rows,
    duplicates whose sum depends on the order).  For bs = 1 .. 8 the blocks read back are invert_blocks(_gather(A)) in bits."""
    name, knobs = case
    A = named_operator(name)
    op = device.DeviceCSR(A, knobs=knobs)
    try:
        sched = op.schedule()
        if name == 'fem12':
            assert sched['sliced_rows'] and sched['window_codes'] and A.shape[0] == 5184
        if name in ('s3_small', 's3_plain'):
            assert sched['value_dict'] == (name == 's3_small')
            assert op.values_route() == ('replanned' if name == 's3_small' else 'in_place')
        if name == 'lap3d':
            assert sched['pattern']
        if name == 'raw':
            assert not sched['sliced_rows'] and not sched['window']
        with pytest.raises(L.PrcgError, match='no block-Jacobi blocks'):
            op.get_block_jacobi(bs=3)
        for bs in range(1, 9):
            op.build_block_jacobi(bs)
            assert same_bits(op.get_block_jacobi(), restatement(name, bs)), (name, bs)
    finally:
        op.close()


@pytest.mark.gpu
@pytest.mark.parametrize('bs', [3, 8])
def test_edge_sizes(bs):
    """n = 1, a single short block, exactly one tile, one row more, two tiles and a short block"""
    tr = 256 - 256 % bs
    for n in (1, bs - 1, tr, tr + 1, 2 * tr + bs - 1):
        A = dominant_spd(n, seed=10 * bs + n % 7)
        want, bad = cgv.invert_blocks(gathered(A, bs))
        assert not bad.any()
        op = device.DeviceCSR(A)
        try:
            op.build_block_jacobi(bs)
            assert same_bits(op.get_block_jacobi(), want), (bs, n)
        finally:
            op.close()


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['fem12', 's3_small'])
def test_after_update_values(name):
    """fem12 in place, s3_small re-planned: the blocks stay frozen until build_block_jacobi is called again, then they are the
    restatement on the new values"""
    A, B = named_operator(name), new_values(name)
    op = device.DeviceCSR(A)
    try:
        op.build_block_jacobi(3)
        old = op.get_block_jacobi()
        assert same_bits(old, restatement(name, 3)) and op._bj_built == 3
        assert op.update_values(B.data) == ('in_place' if name == 'fem12' else 'replanned')
        assert op._bj_built is None and same_bits(op.get_block_jacobi(), old)
        op.build_block_jacobi(3)
        new = op.get_block_jacobi()
        assert same_bits(new, restatement(name, 3, 'new')) and not same_bits(new, old)
    finally:
        op.close()


@pytest.mark.gpu
def test_sessions(monkeypatch):
    """hs_pcg, pr_pcg, pipe_pr_pcg, pipe_p_pcg on fem12 with DeviceBlockJacobi(A, 3): every vector, scalar row, coefficient and
    history is that of the session handed the same inverses through prcg_set_block_jacobi; the matrix is never gathered on the
    host; the blocks are built once for the four solves and again after update_values."""
    from new_cg_variants_amd.callbacks import residual_2_norm, updated_residual_2_norm
    A = operator('fem12').copy()
    n = A.shape[0]
    b, x0 = rhs_for(n)
    want_new = restatement('fem12', 3, 'new')                         # (before _gather is counted)
    gathers, builds = [], []
    real_gather, real_build = cgv.BlockJacobi._gather.__func__, device.DeviceCSR.build_block_jacobi
    monkeypatch.setattr(cgv.BlockJacobi, '_gather', classmethod(lambda cls, *a: gathers.append(1) or real_gather(cls, *a)))
    monkeypatch.setattr(device.DeviceCSR, 'build_block_jacobi', lambda self, bs: builds.append(bs) or real_build(self, bs))
    cgv.clear_operator_cache()
    fresh = device.DeviceCSR(A)
    try:
        P = cgv.DeviceBlockJacobi(A, 3)
        got = {}
        for method in ('hs_pcg', 'pr_pcg', 'pipe_pr_pcg', 'pipe_p_pcg'):
            out = getattr(cgv, method)(A, b, x0, ITERS + 1, callbacks=[updated_residual_2_norm, residual_2_norm], preconditioner=P)
            op = cgv._operator(A, 0)
            assert op.k == ITERS and op._bj_built == 3 and op._bj_bs == 3
            got[method] = read_session(op)
            assert same_bits(out['updated_residual_2_norm'], got[method]['history updated_residual_2_norm None'])
            assert builds == [3], (method, builds)                    # built for the first solve, in force for the others
        assert not gathers and P._inv_blocks is None, 'the device path touched the matrix on the host'
        blocks = P.inv_blocks                                         # the host restatement, now
        assert len(gathers) == 1
        assert same_bits(op.get_block_jacobi(), blocks)
        for method, variant in (('hs_pcg', L.HS), ('pr_pcg', L.PR), ('pipe_pr_pcg', L.PIPE_PR), ('pipe_p_pcg', L.PIPE_P)):
            want = run_session(fresh, variant, b, x0, block_jacobi=(3, blocks))
            assert want['schedule']['block_jacobi']
            assert_same_session(method, got[method], want)
        # a plain session removes the blocks: the next one builds them again
        cgv.pipe_pr_cg(A, b, x0, 5)
        assert op._bj_built is None and not op.schedule()['block_jacobi']
        cgv.pipe_pr_pcg(A, b, x0, 5, preconditioner=P)
        assert builds == [3, 3] and op.schedule()['block_jacobi']
        # new values: update_values leaves the old blocks frozen, the next solve builds the new ones
        A.data[:] = scaled(A).data
        assert cgv.update_values(A) == 'in_place' and cgv._operator(A, 0) is op
        assert op._bj_built is None and same_bits(op.get_block_jacobi(), blocks)
        out = cgv.pipe_pr_pcg(A, b, x0, ITERS + 1, callbacks=[updated_residual_2_norm], preconditioner=cgv.DeviceBlockJacobi(A, 3))
        assert builds == [3, 3, 3] and op._bj_built == 3
        assert same_bits(op.get_block_jacobi(), want_new)
        assert np.all(np.isfinite(out['updated_residual_2_norm'])) and len(gathers) == 1
    finally:
        fresh.close()
        cgv.clear_operator_cache()


@pytest.mark.gpu
@pytest.mark.parametrize('bs', [3, 4, 8])
def test_round_trip(matrices, bs):
    """what prcg_set_block_jacobi was given comes back; whatever surrounded a short last block comes back as the identity"""
    A, _ = matrices['nos7']
    n = A.shape[0]
    assert n == 729
    P = cgv.BlockJacobi(A, bs)
    op = device.DeviceCSR(A)
    try:
        op.set_block_jacobi(bs, P.inv_blocks)
        assert same_bits(op.get_block_jacobi(), P.inv_blocks)
        m = n % bs
        if m:
            junk = P.inv_blocks.copy()
            junk[-1, m:, :] = 7.0
            junk[-1, :, m:] = -3.0
            op.set_block_jacobi(bs, junk)
            assert same_bits(op.get_block_jacobi(), P.inv_blocks)
        # around the wrapper: the C-ABI alone, the caller names bs
        L.check(op._h, op._lib.prcg_set_block_jacobi(op._h, bs, L.ptr(L.f64(P.inv_blocks))))
        assert same_bits(op.get_block_jacobi(bs=bs), P.inv_blocks)
        op.set_block_jacobi(0, None)
        with pytest.raises(L.PrcgError, match='no block-Jacobi blocks'):
            op.get_block_jacobi(bs=bs)
    finally:
        op.close()


@pytest.mark.gpu
def test_a_bad_block_is_reported_and_leaves_no_blocks():
    good = dominant_spd(64, seed=5)
    D = good.toarray()
    D[4:6, 4:6] = 0.0                                                # block 2 at bs = 2
    D[20:22, 20:22] = 0.0                                            # ... and block 10: the smallest index is reported
    A = sp.csr_matrix(D)
    b, x0 = rhs_for(64)
    lib = L.lib()
    op = device.DeviceCSR(A)
    try:
        op.set_block_jacobi(2, np.tile(np.eye(2), (32, 1, 1)))       # blocks set before are dropped by the failing build
        bad = C.c_int64(-5)
        assert lib.prcg_build_block_jacobi(op._h, 2, C.byref(bad)) == L.EINVAL
        assert bad.value == 2
        text = lib.prcg_last_error(op._h).decode()
        assert 'diagonal block 2 (bs = 2) is singular or not finite' in text
        assert lib.prcg_get_block_jacobi(op._h, L.ptr(np.zeros(64 * 8))) == L.EINVAL
        with pytest.raises(ValueError, match=BAD_TEXT.format(2, 2)):
            op.build_block_jacobi(2)
        assert op._bj_built is None and op._bj_bs is None
        L.check(op._h, lib.prcg_solve_begin(op._h, L.HS, L.ptr(b), L.ptr(x0), 5, None, None, 0))
        assert not op.schedule()['block_jacobi']
        with pytest.raises(ValueError, match='DeviceBlockJacobi: ' + BAD_TEXT.format(2, 2)):
            cgv.clear_operator_cache()
            cgv.hs_pcg(A, b, x0, 5, preconditioner=cgv.DeviceBlockJacobi(A, 2))
        # a good operator on the same handle: the build and a solve succeed
        op._set_matrix(good, None)
        bad = C.c_int64(-5)
        assert lib.prcg_build_block_jacobi(op._h, 2, C.byref(bad)) == L.OK and bad.value == -1
        assert lib.prcg_build_block_jacobi(op._h, 2, None) == L.OK   # the pointer is optional
        op._bj_bs = 2
        assert same_bits(op.get_block_jacobi(), cgv.invert_blocks(gathered(good, 2))[0])
        op.begin(L.HS, b, x0, ITERS + 1, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM, block_jacobi=(2, None))
        assert op.schedule()['block_jacobi']
        op.iterate(ITERS)
        op.sync()
        hist = op.history()['updated_residual_2_norm']
        # strictly dominant diagonal, |off-diagonal| row sums s against d = s + [1, 2), s about 6: the Jacobi-scaled spectrum lies in
        # [1 - rho, 1 + rho], rho < 0.9, so 20 CG iterations reduce the error by 2 ((sqrt(19) - 1) / (sqrt(19) + 1))^20 < 2e-4
        assert np.all(np.isfinite(hist)) and hist[ITERS] < 1e-2 * hist[0]
    finally:
        op.close()
        cgv.clear_operator_cache()


@pytest.mark.gpu
def test_refusals_leave_the_handle_as_it_was():
    """argument and state checks only: nothing here reaches a kernel"""
    lib = L.lib()
    # before prcg_set_csr
    h = C.c_void_p()
    assert lib.prcg_create(C.byref(h), 0) == L.OK
    try:
        bad = C.c_int64(5)
        assert lib.prcg_build_block_jacobi(h, 3, C.byref(bad)) == L.EINVAL and b'no operator' in lib.prcg_last_error(h)
        assert lib.prcg_get_block_jacobi(h, L.ptr(np.zeros(9))) == L.EINVAL and b'no block-Jacobi blocks' in lib.prcg_last_error(h)
        assert lib.prcg_values_route(h) == -1
    finally:
        lib.prcg_destroy(h)
    # bs outside 1..8: the blocks in force stay
    A = operator('fem12')
    x = np.random.default_rng(1).standard_normal(A.shape[0])
    op = device.DeviceCSR(A)
    try:
        op.build_block_jacobi(3)
        before, y0 = op.get_block_jacobi(), op.matvec(x)[0]
        for bs in (0, 9, -1):
            with pytest.raises(L.PrcgError, match='outside 1..8') as err:
                op.build_block_jacobi(bs)
            assert err.value.code == L.EINVAL
        assert op._bj_built == 3 and same_bits(op.get_block_jacobi(), before) and same_bits(op.matvec(x)[0], y0)
        assert lib.prcg_get_block_jacobi(op._h, None) == L.EINVAL and b'null output' in lib.prcg_last_error(op._h)
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
            op.build_block_jacobi(3)
        assert err.value.code == L.EINVAL and op._bj_built is None
        assert lib.prcg_get_block_jacobi(op._h, L.ptr(np.zeros(blk.shape[0] * 8 + 64))) == L.EINVAL
        assert same_bits(op.matvec_ext(x_ext), y0)
    finally:
        op.close()
    # a world size > 1 on the handle
    op = device.DeviceCSR(A, world=(0, 2))
    try:
        with pytest.raises(L.PrcgError, match='world size') as err:
            op.build_block_jacobi(3)
        assert err.value.code == L.EINVAL
        assert same_bits(op.matvec(x)[0], A @ x)
    finally:
        op.close()
