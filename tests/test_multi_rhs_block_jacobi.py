"""Block-Jacobi sessions with two and four right-hand sides (prcg.h: prcg_solve_begin_multi_block_jacobi;
DeviceCSR.begin_multi_block_jacobi; cg_variants.hs_bpcg_multi / pr_bpcg_multi / m_bpcg_multi).

Per column the session runs the recurrence of hs_pcg / pr_pcg / m_pcg with M^-1 the point-block Jacobi on the handle, whose
arithmetic BlockJacobi.__call__ / VarBlockJacobi.__call__ carry bit for bit, and every inner product is summed in a fixed order:
those of the block launches in the tree tests/multi_block_common.py restates, the others in device_order.device_sum (the harness
shared with the other multi-RHS files: tests/multi_rhs_common.py).  The oracle
(oracle/ne_oracle.py) run with those routed sums is asked for EQUAL BITS: vectors, every scalar row, alpha, beta, the predicted
nu, the history.  np.array_equal with NaN equal to NaN; no tolerance anywhere.

The oracle runs are computed once per case and shared; nobody writes to them.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from device_order import device_sum
from multi_block_common import (BlockTree, assert_column_bits, assert_finite_nonzero, device_columns, greedy_tiles, oracle_column,
                                uniform_partition, uniform_tiles)
from multi_rhs_common import amd, two_rhs      # noqa: F401  (amd: the fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = 'prcg_solve_begin_multi_block_jacobi'


# ---------------------------------------------------------------------------------------------------------------- CPU
def test_header_binding_and_export():
    from new_cg_variants_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'prcg.h')).read()
    assert re.search(r'int\s+' + ENTRY + r'\s*\(\s*prcg_t\s*\*\s*h,\s*int variant,\s*int nrhs,\s*const double\s*\*\s*const\s*\*\s*b,'
                     r'\s*const double\s*\*\s*const\s*\*\s*x0,\s*int max_iter,\s*uint32_t hist_mask\s*\)\s*;', header)
    res, args = _lib._SIGNATURES[ENTRY]
    assert res is C.c_int and len(args) == 7 and args[-1] is C.c_uint32
    lib = _lib.lib()
    assert hasattr(lib, ENTRY)
    assert lib.prcg_version() == 1
    syms = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r'\bT ' + ENTRY + r'\b', syms)


@pytest.mark.parametrize('fname,other', [('hs_bpcg_multi', 'hs_pcg_multi'), ('pr_bpcg_multi', 'pr_pcg_multi'), ('m_bpcg_multi', 'm_pcg_multi')])
def test_python_entry_points_check_before_the_device(amd, monkeypatch, fname, other):
    cgv, cbs, P = amd['cgv'], amd['cbs'], amd['problems']
    import new_cg_variants_amd as pkg
    f = getattr(cgv, fname)
    assert fname in cgv.__all__ and callable(f) and f.__name__ == fname
    assert pkg.cg_variants is cgv

    def touched(*a, **k):
        raise AssertionError('the device was touched')
    monkeypatch.setattr(cgv, '_operator', touched)
    A = P.fem_like_3d(3)
    n = A.shape[0]
    bj = cgv.BlockJacobi(A, 3)
    B, X0 = np.ones((2, n)), np.zeros((2, n))
    with pytest.raises(ValueError, match=r'B must have shape'):
        f(A, np.ones((3, n)), np.zeros((3, n)), 5, bj)
    with pytest.raises(ValueError, match=r'B must have shape'):
        f(A, np.ones(n), np.zeros(n), 5, bj)
    with pytest.raises(ValueError, match=r'X0 must have shape'):
        f(A, np.ones((4, n)), np.zeros((2, n)), 5, bj)
    with pytest.raises(ValueError, match=other):
        f(A, B, X0, 5, None)
    with pytest.raises(ValueError, match=other):
        f(A, B, X0, 5, cgv.Jacobi(A))
    with pytest.raises(ValueError, match=other):
        f(A, B, X0, 5, lambda v: 0.5 * v)
    with pytest.raises(ValueError, match='recorder residual_2_norm is not served'):
        f(A, B, X0, 5, bj, callbacks=[cbs.residual_2_norm])
    with pytest.raises(ValueError, match='x_true is not served'):
        f(A, B, X0, 5, bj, x_true=np.zeros(n))
    with pytest.raises(ValueError, match='w_replace is not served'):
        f(A, B, X0, 5, bj, w_replace=lambda **kw: False)
    with pytest.raises(ValueError, match='made for a matrix of'):
        f(A, B, X0, 5, cgv.DeviceBlockJacobi(P.fem_like_3d(2), 3))
    # with every argument in order the next step IS the device
    with pytest.raises(AssertionError, match='the device was touched'):
        f(A, B, X0, 5, bj, callbacks=[cbs.updated_residual_2_norm])
    # the old functions keep their refusal, now with a pointer to the new one
    with pytest.raises(ValueError, match='block-Jacobi preconditioner is not served by the two-RHS session'):
        getattr(cgv, other)(A, B, X0, 5, bj)


@pytest.mark.parametrize('bs', range(1, 9))
def test_model_tiles_of_a_uniform_partition(bs):
    """the greedy tiling of a uniform partition IS the uniform kernels' tiles of 256 - 256 % bs rows, a short last block included --
    unless that short block fits into the lanes a full tile leaves idle: then the greedy tiling takes it in (one tile fewer).
    For those n (n mod tr in 1 .. 256 % bs) the same inverses given as block_jacobi= and as the uniform partition through
    block_jacobi_var= are summed in different trees and need NOT give equal bits; test_invariants compares the two forms at
    n = 12287, which is not such an n."""
    tr = 256 - 256 % bs
    assert np.array_equal(uniform_tiles(5 * tr, bs), np.arange(6) * tr)
    for n in (1, bs, tr - 1, tr, tr + bs, tr + bs + 1, 3 * tr + 9 * bs - 1, 60000, 90000, 2100000):
        if 0 < n % tr <= 256 % bs:
            continue
        assert np.array_equal(greedy_tiles(uniform_partition(n, bs)), uniform_tiles(n, bs)), (bs, n)
    for spill in range(1, 256 % bs + 1):                       # the exception: n = 2 tiles and a block of `spill` rows
        n = 2 * tr + spill
        assert np.array_equal(greedy_tiles(uniform_partition(n, bs)), [0, tr, n])
        assert np.array_equal(uniform_tiles(n, bs), [0, tr, 2 * tr, n])


def test_model_sums_every_row_once_and_is_its_own_tree():
    sizes = np.resize(np.arange(1, 9), 700)                                # the cyclic partition 1, 2, .., 8, 1, ..
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    tree = BlockTree(ptr)
    n = tree.n
    assert tree.ntiles > 1 and (np.diff(tree.tile_rows) <= 256).all()
    assert np.isin(tree.tile_rows, ptr).all(), 'a tile holds whole blocks'
    count = np.zeros(n, dtype=np.int64)
    np.add.at(count, tree.idx[tree.live], 1)
    assert (count == 1).all()
    powers = 2.0 ** (np.arange(n) % 40)                                    # exact in any order: the sum counts every row once
    assert tree(powers) == powers.sum() == np.float64(sum(int(q) for q in powers))
    crafted = np.resize(np.array([1e16, 1.0, -1e16, 1.0, 1.0]), n)         # order matters here
    assert tree(crafted) != device_sum(crafted), 'the block tree is not device_sum: routing the sums matters'
    uni = BlockTree(n=n, bs=3)
    assert uni(crafted) != device_sum(crafted)


# ---------------------------------------------------------------------------------------------------------------- GPU
def cyclic_partition(n):
    sizes = np.resize(np.arange(1, 9), n)
    ptr = np.concatenate([[0], np.cumsum(sizes)])
    ptr = ptr[ptr < n]
    return np.concatenate([ptr, [n]]).astype(np.int64)


@functools.lru_cache(maxsize=None)
def matrix(name):
    from new_cg_variants_amd import problems as P
    if name == 'fem16':
        return P.fem_like_3d(16, 3)
    if name == 'fem_irregular20':
        return P.fem_irregular_3d(20)
    if name == 'lap300x200':
        return P.laplace_2d(300, 200)
    if name == 'lap300x300':
        return P.laplace_2d(300, 300)
    if name == 'lap1500x1400':
        return P.laplace_2d(1500, 1400)
    from conftest import load_matrix
    return load_matrix(name)[0]


@functools.lru_cache(maxsize=None)
def problem(name):
    from new_cg_variants_amd import problems as P
    A = matrix(name)
    B = two_rhs(P, A)
    B.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def preconditioner(name, kind):
    """(the host object whose __call__ carries the device's bits, the partition, begin's block argument as a dict)"""
    import new_cg_variants_amd.cg_variants as cgv
    from new_cg_variants_amd import problems as P
    A = matrix(name)
    n = A.shape[0]
    if kind.startswith('bs'):                          # 'bs3' set from the host, 'bs3dev' built on the device
        bs = int(kind[2])
        if kind.endswith('dev'):
            obj = cgv.DeviceBlockJacobi(A, bs)
            return obj, uniform_partition(n, bs), dict(block_jacobi=(bs, None))
        obj = cgv.BlockJacobi(A, bs)
        return obj, uniform_partition(n, bs), dict(block_jacobi=(bs, obj.inv_blocks))
    ptr = {'irregular': lambda: P.fem_irregular_blocks(20), 'cyclic': lambda: cyclic_partition(n)}[kind.replace('dev', '')]()
    ptr = np.asarray(ptr, dtype=np.int64)
    if kind.endswith('dev'):
        obj = cgv.DeviceVarBlockJacobi(A, ptr)
        return obj, ptr, dict(block_jacobi_var=(ptr, None))
    obj = cgv.VarBlockJacobi(A, ptr)
    return obj, ptr, dict(block_jacobi_var=(ptr, obj.inv_blocks))


@functools.lru_cache(maxsize=None)
def reference(name, kind, variant, iters, column):
    A, B = problem(name)
    obj, ptr, _ = preconditioner(name, kind)
    tree = BlockTree(n=A.shape[0], bs=int(kind[2])) if kind.startswith('bs') else BlockTree(ptr)
    return oracle_column(A, B[column], np.zeros(A.shape[0]), iters, variant, obj, tree)


KNOBS = {'fem16_csr': {'PRCG_SELL': '0'}}

# (variant, operator, blocks, iterations).  60 iterations where the oracle run allows it; every case asserts its oracle sums finite
# and nonzero.  At least one case per variant and family; every pair is one reference_rhs column and one random column.
CASES = [('hs', 'fem16', 'bs3', 60), ('pr', 'fem16', 'bs3', 60), ('m', 'fem16', 'bs3', 60),
         ('hs', 'fem16', 'bs3dev', 60), ('pr', 'fem16', 'bs3dev', 60),
         ('hs', 'fem16_csr', 'bs3', 60), ('pr', 'fem16_csr', 'bs3', 60),
         ('hs', 'fem_irregular20', 'irregular', 60), ('pr', 'fem_irregular20', 'irregular', 60), ('m', 'fem_irregular20', 'irregulardev', 60),
         ('hs', 'fem_irregular20', 'irregulardev', 60),
         ('hs', 'bcsstk14', 'bs3', 60), ('pr', 'bcsstk14', 'bs3', 60),
         ('hs', 'lap300x200', 'bs7', 60), ('m', 'lap300x200', 'bs7', 60),
         ('hs', 'lap300x300', 'bs3', 60), ('pr', 'lap300x300', 'bs3', 60),
         ('hs', 'bcsstk03', 'bs3', 60), ('pr', 'bcsstk03', 'cyclic', 60)]


def run_case(amd, variant, name, kind, iters, chunks=(1, 2, 7)):
    L = amd['L']
    mat = name.replace('_csr', '')
    A, B = problem(mat)
    n = A.shape[0]
    obj, ptr, blocks = preconditioner(mat, kind)
    want = [reference(mat, kind, variant, iters, j) for j in range(2)]
    for j in range(2):
        assert_finite_nonzero(want[j], f'{variant} {name} {kind} column {j}', variant == 'hs')
    op = amd['device'].DeviceCSR(A, knobs=KNOBS.get(name))
    try:
        got, sched = device_columns(op, L, variant, B, np.zeros((2, n)), iters, chunks=chunks, **blocks)
        if kind.endswith('dev'):                       # the blocks the device built are those of the host restatement
            back = op.get_block_jacobi() if 'block_jacobi' in blocks else op.get_block_jacobi_var()
            assert np.array_equal(np.asarray(back).reshape(-1), np.asarray(obj.inv_blocks).reshape(-1))
    finally:
        op.close()
    assert sched['rhs2'] and not sched['rhs4'] and sched['block_jacobi'] and not sched['small'] and not sched['fused'], sched
    assert sched['block_jacobi_var'] == ('block_jacobi_var' in blocks), sched
    if name.endswith('_csr'):
        assert not sched['sliced_rows'] and not sched['window'], sched
    for j in range(2):
        assert_column_bits(got[j], want[j], f'{variant} {name} {kind} column {j}')
    return sched


@pytest.mark.gpu
@pytest.mark.parametrize('variant,name,kind,iters', CASES)
def test_whole_runs_against_the_oracle(amd, variant, name, kind, iters):
    """Both columns against two oracle runs with M^-1 the same blocks and the sums routed to the device's trees: x, r, p, s, r~,
    (s~), every scalar row, alpha, beta, the predicted nu, the history -- equal bits."""
    if name == 'lap300x200':
        n = matrix(name).shape[0]
        assert n == 60000 == 8571 * 7 + 3, 'a short last block'
    if name == 'lap300x300':
        assert BlockTree(n=90000, bs=3).ntiles == 353 > 256, "the final tree's second round"
    if name == 'bcsstk03':
        assert matrix(name).shape[0] == 112 == 37 * 3 + 1
    sched = run_case(amd, variant, name, kind, iters)
    print(f'{variant} {name} {kind}: {iters} iterations, both columns bit-exact; schedule {sched}')


@pytest.mark.gpu
def test_more_tiles_than_the_handles_partial_rows(amd):
    """laplace_2d(1500, 1400), bs = 8: 8204 tiles, more than the 8192 rows of the handle's own partial arrays -- the session's
    partial arrays are sized from the tile count.  Hestenes-Stiefel, 3 iterations against the oracle."""
    A = matrix('lap1500x1400')
    assert A.shape[0] == 2100000 and BlockTree(n=2100000, bs=8).ntiles == 8204 > 8192
    run_case(amd, 'hs', 'lap1500x1400', 'bs8', 3, chunks=(2, 1))


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['hs', 'pr'])
@pytest.mark.parametrize('name', ['fem16', 'lap300x200'])
def test_four_right_hand_sides_are_two_pairs(amd, variant, name):
    """Columns (0, 1) and (2, 3) of a four-RHS block session equal two two-RHS block sessions begun with those pairs, bit for bit;
    on the sliced-row operator the product of an iteration is one four-vector launch."""
    L = amd['L']
    A, B = problem(name)
    n = A.shape[0]
    kind = 'bs3' if name == 'fem16' else 'bs7'
    _, _, blocks = preconditioner(name, kind)
    B4 = np.stack([B[0], B[1], 0.5 * B[0] + B[1], np.random.default_rng(3).standard_normal(n)])
    X4 = np.zeros((4, n))
    iters = 20
    op = amd['device'].DeviceCSR(A)
    try:
        four, sched = device_columns(op, L, variant, B4, X4, iters, **blocks)
        pairs = [device_columns(op, L, variant, B4[2 * g:2 * g + 2], X4[:2], iters, **blocks)[0] for g in range(2)]
    finally:
        op.close()
    assert sched['rhs4'] and not sched['rhs2'] and sched['block_jacobi'], sched
    assert sched['spmm4'] == sched['sliced_rows'], sched
    if name == 'fem16':
        assert sched['sliced_rows'] and sched['spmm4'], sched
    else:
        assert sched['window'], sched
    for j in range(4):
        assert np.isfinite(four[j]['scalars']).all()
        assert_column_bits(four[j], pairs[j // 2][j % 2], f'{variant} {name}: column {j} of four vs its pair session')


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['hs', 'pr', 'm'])
def test_invariants(amd, variant):
    """Swapped right-hand sides swap the bits; a NaN in b[1] stays in column 1; a uniform partition through block_jacobi_var= is
    block_jacobi= with the same inverses (n = 12287 = 4095 * 3 + 2: a short last block); two runs give equal bits."""
    L, cgv, P = amd['L'], amd['cgv'], amd['problems']
    A = P.fem_like_3d(16, 3)[:12287, :12287].tocsr()             # a principal submatrix: SPD, the last block has two rows
    n = A.shape[0]
    assert n == 12287 == 4095 * 3 + 2
    B = two_rhs(P, A)
    X0 = np.zeros((2, n))
    bj = cgv.BlockJacobi(A, 3)
    ptr = uniform_partition(n, 3)
    packed = np.concatenate([bj.inv_blocks[:-1].reshape(-1), bj.inv_blocks[-1, :2, :2].reshape(-1)])
    iters = 25
    Bnan = B.copy()
    Bnan[1, 5] = np.nan
    op = amd['device'].DeviceCSR(A)
    try:
        ab, _ = device_columns(op, L, variant, B, X0, iters, block_jacobi=(3, bj.inv_blocks))
        again, _ = device_columns(op, L, variant, B, X0, iters, block_jacobi=(3, bj.inv_blocks))
        ba, _ = device_columns(op, L, variant, B[::-1], X0, iters, block_jacobi=(3, bj.inv_blocks))
        nan, _ = device_columns(op, L, variant, Bnan, X0, iters, block_jacobi=(3, bj.inv_blocks))
        var, sched = device_columns(op, L, variant, B, X0, iters, block_jacobi_var=(ptr, packed))
    finally:
        op.close()
    assert sched['block_jacobi_var']
    assert np.isfinite(ab[0]['scalars']).all() and np.isfinite(ab[1]['scalars']).all()
    for j in range(2):
        assert_column_bits(again[j], ab[j], f'{variant}: second run, column {j}')
        assert_column_bits(ba[1 - j], ab[j], f'{variant}: swapped right-hand sides, column {j}')
        assert_column_bits(var[j], ab[j], f'{variant}: the uniform partition as block_jacobi_var=, column {j}')
    assert_column_bits(nan[0], ab[0], f'{variant}: column 0 beside a column with a NaN')
    assert np.isnan(nan[1]['hist'][1:]).all() and np.isnan(nan[1]['x']).any()


def single_block_session(op, L, variant, b, iters, blocks):
    op.begin(variant, b, np.zeros(op.n), iters + 1, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM, **blocks)
    op.iterate(iters)
    op.sync()
    return ({v: op.get_vector(v) for v in ('x', 'r', 'p', 's', 'rt')}, np.array([op.get_scalars(k) for k in range(iters + 1)]),
            op.history()['updated_residual_2_norm'])


@pytest.mark.gpu
@pytest.mark.parametrize('variant', ['hs', 'pr'])
def test_life_cycle_on_one_handle(amd, variant):
    """Jacobi two-RHS session, block session, single block-Jacobi session, block session again on ONE handle: each carries the bits
    it has alone.  After update_values and build_block_jacobi the block session equals a fresh handle's; after set_csr the new
    begin is refused for lack of blocks."""
    L, P = amd['L'], amd['problems']
    A, B = problem('fem16')
    n = A.shape[0]
    X0 = np.zeros((2, n))
    code = {'hs': L.HS, 'pr': L.PR}[variant]
    _, _, blocks = preconditioner('fem16', 'bs3')
    dev = dict(block_jacobi=(3, None))
    iters = 12
    mask = L.HIST_UPDATED_RESIDUAL_2_NORM

    def jacobi_session(op):
        op.clear_preconditioners()
        op.begin_multi(code, B, X0, iters + 1, inv_diag=1 / A.diagonal(), hist_mask=mask)
        op.iterate(iters)
        op.sync()
        return [(op.get_vector('x', rhs=j), op.history(rhs=j)['updated_residual_2_norm']) for j in range(2)]

    op, fresh = amd['device'].DeviceCSR(A), amd['device'].DeviceCSR(A)
    try:
        alone_block, _ = device_columns(fresh, L, variant, B, X0, iters, **blocks)
        alone_single = single_block_session(fresh, L, code, B[0], iters, blocks)
        alone_jacobi = jacobi_session(fresh)
        jac = jacobi_session(op)
        first, sched = device_columns(op, L, variant, B, X0, iters, **blocks)
        single = single_block_session(op, L, code, B[0], iters, blocks)
        assert op.schedule()['block_jacobi'] and not op.schedule()['rhs2']
        second, _ = device_columns(op, L, variant, B, X0, iters, **blocks)
        for j in range(2):
            assert np.array_equal(jac[j][0], alone_jacobi[j][0]) and np.array_equal(jac[j][1], alone_jacobi[j][1])
            assert_column_bits(first[j], alone_block[j], f'{variant}: block session after a Jacobi session, column {j}')
            assert_column_bits(second[j], alone_block[j], f'{variant}: block session after a single block session, column {j}')
        for v in single[0]:
            assert np.array_equal(single[0][v], alone_single[0][v]), v
        assert np.array_equal(single[1], alone_single[1]) and np.array_equal(single[2], alone_single[2])
        # a Newton step: new values on the pattern, blocks rebuilt on the device, the new begin
        A2 = A.copy()
        A2.data = A.data * 1.5
        op.update_values(A2.data)
        op.build_block_jacobi(3)
        newton, _ = device_columns(op, L, variant, B, X0, iters, **dev)
        fresh2 = amd['device'].DeviceCSR(A2)
        try:
            want, _ = device_columns(fresh2, L, variant, B, X0, iters, **dev)
        finally:
            fresh2.close()
        for j in range(2):
            assert_column_bits(newton[j], want[j], f'{variant}: after update_values and build_block_jacobi, column {j}')
        # a new operator drops the blocks: the entry itself refuses
        op._set_matrix(A, None)
        bp = (C.c_void_p * 2)(B[0].ctypes.data, B[1].ctypes.data)
        rc = L.lib().prcg_solve_begin_multi_block_jacobi(op._h, code, 2, bp, bp, 5, 0)
        assert rc == L.EINVAL and b'no block-Jacobi preconditioner is set' in L.lib().prcg_last_error(op._h)
    finally:
        op.close()
        fresh.close()
    assert sched['rhs2'] and sched['block_jacobi']


def _refused(L, op, text, variant, nrhs, b, x0, max_iter, mask):
    rc = L.lib().prcg_solve_begin_multi_block_jacobi(op._h, variant, nrhs, b, x0, max_iter, mask)
    msg = L.lib().prcg_last_error(op._h).decode()
    assert rc == L.EINVAL and text in msg and msg.startswith(ENTRY + ':'), (rc, msg)


@pytest.mark.gpu
def test_refusals(amd):
    """Every refusal of the entry with its text; the old entries keep theirs while blocks are set; schedule() reports the session;
    the single-column accessors and the vectors the session does not keep are refused while it is open."""
    L, P, cgv = amd['L'], amd['problems'], amd['cgv']
    A, B = problem('fem16')
    n = A.shape[0]
    B = np.ascontiguousarray(B)
    X0 = np.zeros((2, n))
    bj, ptr, blocks = preconditioner('fem16', 'bs3')
    lib = L.lib()
    two = (C.c_void_p * 2)(B[0].ctypes.data, B[1].ctypes.data)
    three = (C.c_void_p * 3)(B[0].ctypes.data, B[1].ctypes.data, B[0].ctypes.data)
    holed = (C.c_void_p * 2)(B[0].ctypes.data, None)
    empty = C.c_void_p()
    assert lib.prcg_create(C.byref(empty), 0) == 0
    try:
        _refused(L, type('H', (), {'_h': empty}), 'call prcg_set_csr first', L.HS, 2, two, two, 8, 0)
    finally:
        lib.prcg_destroy(empty)
    op = amd['device'].DeviceCSR(A)
    try:
        _refused(L, op, 'no block-Jacobi preconditioner is set', L.HS, 2, two, two, 8, 0)
        op.set_block_jacobi(3, bj.inv_blocks)
        # an open session survives every refusal
        op.begin_multi_block_jacobi(L.PR, B, X0, 9, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM, **blocks)
        op.iterate(2)
        for v in (L.PIPE_PR, L.PIPE_PR_M, L.PIPE_P, L.PIPE_P_M):
            _refused(L, op, 'the pipelined variants are not served with blocks (a follow-up', v, 2, two, two, 8, 0)
        for v in (L.CG_CG, L.GV, 99):
            _refused(L, op, 'serves PRCG_HS (hs_pcg), PRCG_PR (pr_pcg) and PRCG_M (m_pcg) only', v, 2, two, two, 8, 0)
        _refused(L, op, 'nrhs = 3', L.HS, 3, three, three, 8, 0)
        _refused(L, op, 'nrhs = 1', L.HS, 1, two, two, 8, 0)
        _refused(L, op, 'history bits other than PRCG_HIST_UPDATED_RESIDUAL_2_NORM', L.HS, 2, two, two, 8, L.HIST_RESIDUAL_2_NORM)
        _refused(L, op, 'null b or x0', L.HS, 2, None, two, 8, 0)
        _refused(L, op, 'null b or x0', L.HS, 2, two, holed, 8, 0)
        _refused(L, op, 'max_iter must be >= 1', L.HS, 2, two, two, 0, 0)
        op.set_replace_hook(lambda k: False)
        _refused(L, op, 'replace hook', L.HS, 2, two, two, 8, 0)
        op.set_replace_hook(None)
        # the old entries keep refusing a handle with blocks, in their own words
        for begin in (lambda: op.begin_multi(L.HS, B, X0, 8), lambda: op.begin_multi(L.PR, B, X0, 8)):
            with pytest.raises(L.PrcgError, match=r'prcg_solve_begin_multi: a block-Jacobi preconditioner is set'):
                begin()
        with pytest.raises(L.PrcgError, match=r'prcg_solve_begin_multi_pipe: a block-Jacobi preconditioner is set'):
            op.begin_multi_pipe(L.PIPE_PR, B, X0, 8)
        for name in ('hs_pcg_multi', 'pr_pcg_multi', 'm_pcg_multi', 'pipe_pr_pcg_multi'):
            with pytest.raises(ValueError, match='block-Jacobi preconditioner is not served by the two-RHS session'):
                getattr(cgv, name)(A, B, X0, 5, preconditioner=bj)
        # ... and the session that was open is intact
        sched = op.schedule()
        assert sched['rhs2'] and sched['block_jacobi'] and not sched['block_jacobi_var'] and not sched['rhs4'] and not sched['spmm4'], sched
        for call in (lambda: op.get_vector('x'), lambda: op.set_vector('x', B[0]), lambda: op.get_scalars(1),
                     lambda: op.set_scalars(1, np.zeros(L.NUM_SCALARS)), lambda: op.get_coefficients(1),
                     lambda: op.history(), lambda: op.set_iteration(1)):
            with pytest.raises(L.PrcgError, match='two right-hand sides'):
                call()
        for v in ('wt', 'ut', 'w', 'u'):
            with pytest.raises(L.PrcgError, match='not part of the two-RHS session'):
                op.get_vector(v, rhs=0)
        with pytest.raises(L.PrcgError, match='right-hand side 2 out of range'):
            op.get_vector('x', rhs=2)
        op.iterate(1)
        op.sync()
        assert op.k == 3 and np.isfinite(op.get_vector('st', rhs=1)).all()
        # Hestenes-Stiefel keeps no s~
        op.begin_multi_block_jacobi(L.HS, B, X0, 4, **blocks)
        with pytest.raises(L.PrcgError, match='not part of the two-RHS session'):
            op.get_vector('st', rhs=0)
        # a partition reports its bit; four right-hand sides theirs
        pv = cgv.VarBlockJacobi(A, ptr)
        B4, X4 = np.concatenate([B, B]), np.zeros((4, n))
        op.begin_multi_block_jacobi(L.HS, B4, X4, 4, block_jacobi_var=(ptr, pv.inv_blocks))
        sched = op.schedule()
        assert sched['rhs4'] and not sched['rhs2'] and sched['block_jacobi'] and sched['block_jacobi_var'] and sched['spmm4'] == sched['sliced_rows'], sched
        with pytest.raises(ValueError, match='exactly one of block_jacobi= and block_jacobi_var='):
            op.begin_multi_block_jacobi(L.HS, B, X0, 4)
        # a later ordinary begin opens an ordinary session
        op.begin(L.HS, B[0], X0[0], 4)
        assert not op.schedule()['rhs4'] and not op.schedule()['rhs2'] and not op.schedule()['block_jacobi']
    finally:
        op.close()
    ghost = amd['device'].DeviceCSR(sp.hstack([A, sp.csr_matrix((n, 5))]).tocsr())
    try:
        ghost.set_block_jacobi(3, bj.inv_blocks)
        _refused(L, ghost, 'n_ghost = 5 > 0', L.HS, 2, two, two, 8, 0)
    finally:
        ghost.close()


@pytest.mark.gpu
def test_refused_with_a_communicator(amd):
    """A communicator on the handle -- even of one rank -- selects the multi-rank schedules (and such a handle takes no blocks)."""
    from test_distributed import rccl_ids
    L = amd['L']
    A, B = problem('fem16')
    n = A.shape[0]
    B = np.ascontiguousarray(B)
    two = (C.c_void_p * 2)(B[0].ctypes.data, B[1].ctypes.data)
    uid, path = rccl_ids(1)
    comm = amd['device'].DeviceCSR(A, comm_init=(0, 1, uid, path))
    try:
        _refused(L, comm, 'a communicator is set on the handle', L.HS, 2, two, two, 8, 0)
    finally:
        comm.close()


@pytest.mark.gpu
def test_bpcg_multi_returns_trials(amd):
    """cg_variants.hs_bpcg_multi / pr_bpcg_multi: trial dicts whose histories are the session's, for every accepted preconditioner"""
    L, cgv, cbs = amd['L'], amd['cgv'], amd['cbs']
    A, B = problem('fem16')
    n = A.shape[0]
    X0 = np.zeros((2, n))
    iters = 15
    tree = BlockTree(n=n, bs=3)
    assert np.array_equal(tree.tile_rows, BlockTree(uniform_partition(n, 3)).tile_rows)
    carrier = type('Carrier', (), {})()
    carrier.bs, carrier.inv_blocks = 3, cgv.BlockJacobi(A, 3).inv_blocks
    for prec in (cgv.BlockJacobi(A, 3), cgv.DeviceBlockJacobi(A, 3), cgv.VarBlockJacobi(A, uniform_partition(n, 3)),
                 cgv.DeviceVarBlockJacobi(A, uniform_partition(n, 3)), carrier):
        out = cgv.pr_bpcg_multi(A, B, X0, iters + 1, prec, callbacks=[cbs.updated_residual_2_norm])
        assert len(out) == 2 and out[0]['name'] == 'pr_bpcg_multi' and out[1]['rhs'] == 1
        call = cgv.BlockJacobi(A, 3) if prec is carrier else prec        # (the object whose __call__ carries these blocks' bits)
        for j in range(2):
            want = oracle_column(A, B[j], X0[j], iters, 'pr', call, tree)['hist']
            assert np.array_equal(out[j]['updated_residual_2_norm'], want), (type(prec).__name__, j)
    out4 = cgv.hs_bpcg_multi(A, np.concatenate([B, B]), np.zeros((4, n)), 8, cgv.BlockJacobi(A, 3), callbacks=[cbs.updated_residual_2_norm])
    assert len(out4) == 4 and np.array_equal(out4[0]['updated_residual_2_norm'], out4[2]['updated_residual_2_norm'])
    cgv.clear_operator_cache()
