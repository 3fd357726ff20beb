"""TEST INFRASTRUCTURE of tests/test_multi_rhs_block_jacobi.py: the summation tree of the block launches of a block-Jacobi session
with two or four right-hand sides (new_cg_variants_amd/csrc/prcg_blockjac.hip: k_block_jacobi_dots / k_block_jacobi_var_dots),
restated in NumPy, and the oracle runs routed through it (the oracle column and the session read-out themselves are the shared ones
of tests/multi_rhs_common.py).

  tiles  : the partition cut greedily into runs of consecutive whole blocks with at most 256 rows (prcg_bjvar.h: bjvar_plan); a
           uniform block size bs: tiles of 256 - 256 % bs rows, which are the greedy tiles of the partition 0, bs, 2 bs, .., n
           (uniform_tiles names the one exception)
  lane   : lane t of tile T holds the product of row tile_row0[T] + t; a lane without a row holds +0.0
  wave   : xor butterfly 32, 16, 8, 4, 2, 1          workgroup: waves 0..3 in order  ->  ONE partial per tile
  final  : the 256-thread tree over the tile partials in tile order (device_order._final_tree)

Which sum follows which tree (prcg.h: prcg_solve_begin_multi_block_jacobi):
  Hestenes-Stiefel   nu and the recorded r.r: the block tree;  mu: device_sum (k_hs2_dot_ps)
  PR / M             mu, delta, gamma: the block tree, always;  nu and r.r: the block tree at the start, device_sum (k_pr2_update)
                     in every later iteration
"""
import numpy as np

import multi_rhs_common as common
import oracle.ne_oracle as orc
from device_order import Routed, _butterfly, _final_tree, device_sum
from multi_rhs_common import KEYS, assert_column_bits      # noqa: F401  (for tests/test_multi_rhs_block_jacobi.py)

LANES = 256


def uniform_partition(n, bs):
    return np.concatenate([np.arange(0, n, bs), [n]]).astype(np.int64)


def greedy_tiles(block_ptr):
    """first row of every tile, and n: a tile closes when the next block would not fit into 256 rows"""
    ptr = np.asarray(block_ptr, dtype=np.int64)
    assert ptr[0] == 0 and (np.diff(ptr) >= 1).all() and (np.diff(ptr) <= 8).all()
    nb, k, rows = ptr.size - 1, 0, []
    while k < nb:
        rows.append(int(ptr[k]))
        k = int(np.searchsorted(ptr, ptr[k] + LANES, side='right')) - 1      # the last boundary within 256 rows of the tile's first
    return np.array(rows + [int(ptr[-1])], dtype=np.int64)


def uniform_tiles(n, bs):
    """first row of every tile of the uniform kernels, and n: tiles of 256 - 256 % bs rows.  These ARE greedy_tiles of the uniform
    partition, except where a short last block fits into the lanes a full tile leaves idle (n % tr <= 256 % bs): the greedy tiling
    then takes it into the last full tile, the uniform kernels give it a tile of its own."""
    tr = LANES - LANES % bs
    return np.concatenate([np.arange(0, n, tr), [n]]).astype(np.int64)


class BlockTree:
    """sum(prod) in the order of a block launch: over the tiles of a partition (block_ptr=) or of a uniform block size (n=, bs=)"""

    def __init__(self, block_ptr=None, n=None, bs=None):
        self.tile_rows = greedy_tiles(block_ptr) if block_ptr is not None else uniform_tiles(n, bs)
        self.n = int(self.tile_rows[-1])
        first, count = self.tile_rows[:-1], np.diff(self.tile_rows)
        assert (count >= 1).all() and (count <= LANES).all()
        lane = np.arange(LANES)
        self.idx = first[:, None] + lane[None, :]
        self.live = lane[None, :] < count[:, None]
        self.idx[~self.live] = 0

    @property
    def ntiles(self):
        return self.idx.shape[0]

    def __call__(self, prod):
        prod = np.asarray(prod, dtype=np.float64)
        assert prod.shape == (self.n,)
        vals = np.where(self.live, prod[self.idx], 0.0)                       # a lane without a row adds +0.0
        waves = _butterfly(vals.reshape(self.ntiles, 4, 64))
        partial = waves[:, 0]
        for w in range(1, 4):
            partial = partial + waves[:, w]
        return _final_tree(partial)


def oracle_column(A, b, x0, iters, variant, prec, tree):
    """hs_pcg / pr_pcg / m_pcg of the oracle with M^-1 = `prec` and every inner product routed to the tree the device sums it with:
    the state after `iters` iterations, the scalars of every iteration, the coefficients used BY every iteration >= 1, the history.
    Scalars: [mu, delta, gamma, nu, rr] (Hestenes-Stiefel: delta = gamma = 0)."""
    hs = variant == 'hs'
    if hs:
        dot = Routed(tree, device_sum)                    # nu, mu -- at the start and in every advance
        dot0 = dot
    else:
        dot = Routed(tree, tree, tree, device_sum)        # advance: mu, delta, gamma, nu
        dot0 = Routed(tree)                               # start: nu, mu, delta, gamma, all from block launches
    method = {'hs': orc.hs_pcg, 'pr': orc.pr_pcg, 'm': orc.m_pcg}[variant]
    return common.oracle_column(method, A, b, x0, iters, tilde=('rt',) if hs else ('rt', 'st'),
                                rr=lambda st: np.float64((tree if (hs or st.k == 0) else device_sum)(st.r * st.r)),
                                preconditioner=prec, dot=dot, dot0=dot0, square=lambda a: a * a)


def device_columns(op, L, variant, B, X0, iters, chunks=(1, 2, 7), **blocks):
    """A block-Jacobi multi-RHS session on `op` read through the per-column getters; blocks: block_jacobi= or block_jacobi_var="""
    hs = variant == 'hs'

    def begin():
        op.begin_multi_block_jacobi({'hs': L.HS, 'pr': L.PR, 'm': L.M}[variant], B, X0, iters + 1, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM,
                                    **blocks)
    return common.device_columns(op, L, begin, iters, np.asarray(B).shape[0], common.VECS + (('rt',) if hs else ('rt', 'st')),
                                 common.served_slots(L, hs), chunks, report=common.served_slots(L, False))


def assert_finite_nonzero(want, what, hs):
    """every oracle inner product of every compared iteration is finite and nonzero (a case that breaks down is a wrong case)"""
    sc = want['scalars'][:, [0, 3, 4]] if hs else want['scalars']
    assert np.isfinite(sc).all() and (sc != 0).all(), f'{what}: an oracle inner product is zero or not finite'
    assert np.isfinite(want['x']).all(), what
