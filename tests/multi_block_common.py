"""TEST INFRASTRUCTURE of tests/test_multi_rhs_block_jacobi.py: the summation tree of the block launches of a block-Jacobi session
with two or four right-hand sides (new_cg_variants_amd/csrc/prcg_blockjac.hip: k_block_jacobi_dots / k_block_jacobi_var_dots),
restated in NumPy, and the oracle runs routed through it.

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

import oracle.ne_oracle as orc
from device_order import Routed, _butterfly, _final_tree, device_sum

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
    rows = []
    hs = variant == 'hs'

    def tap(st):
        rr_sum = tree if (hs or st.k == 0) else device_sum
        rr = np.float64(rr_sum(st.r * st.r))
        rows.append((st.mu, 0.0 if hs else st.dl, 0.0 if hs else st.gm, st.nu, rr, st.alpha, st.beta, 0.0 if hs else st.nu_pred))

    if hs:
        dot = Routed(tree, device_sum)                    # nu, mu -- at the start and in every advance
        dot0 = dot
    else:
        dot = Routed(tree, tree, tree, device_sum)        # advance: mu, delta, gamma, nu
        dot0 = Routed(tree)                               # start: nu, mu, delta, gamma, all from block launches
    method = {'hs': orc.hs_pcg, 'pr': orc.pr_pcg, 'm': orc.m_pcg}[variant]
    with np.errstate(all='ignore'):
        out = method(A, b, x0, iters + 1, preconditioner=prec, dot=dot, dot0=dot0, square=lambda a: a * a, tap=tap)
        st = out['_final_state']
        rows = np.array(rows)
        res = {'x': st.x, 'r': st.r, 'p': st.p, 's': st.s, 'rt': st.rt, 'st': None if hs else st.st,
               'scalars': rows[:, :5], 'alpha': rows[:-1, 5], 'beta': rows[1:, 6], 'nu_pred': rows[1:, 7], 'hist': np.sqrt(rows[:, 4])}
    for v in res.values():
        if v is not None:
            v.setflags(write=False)
    return res


def device_columns(op, L, variant, B, X0, iters, chunks=(1, 2, 7), **blocks):
    """A block-Jacobi multi-RHS session on `op` read through the per-column getters; blocks: block_jacobi= or block_jacobi_var="""
    code = {'hs': L.HS, 'pr': L.PR, 'm': L.M}[variant]
    op.begin_multi_block_jacobi(code, B, X0, iters + 1, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM, **blocks)
    sched = op.schedule()
    for c in chunks:                                    # calls of any length give the same session
        op.iterate(min(c, iters - op.k))
    op.iterate(iters - op.k)
    op.sync()
    assert op.k == iters
    hs = variant == 'hs'
    served = (L.S_MU, L.S_NU, L.S_RR) if hs else (L.S_MU, L.S_DELTA, L.S_GAMMA, L.S_NU, L.S_RR)
    cols = []
    for j in range(np.asarray(B).shape[0]):
        sc = np.array([op.get_scalars(k, rhs=j) for k in range(iters + 1)])
        other = [q for q in range(L.NUM_SCALARS) if q not in served]
        assert not sc[:, other].any(), 'slots the session does not serve are 0'
        cf = np.array([op.get_coefficients(k, rhs=j) for k in range(1, iters + 1)]).reshape(iters, 3)
        col = {v: op.get_vector(v, rhs=j) for v in ('x', 'r', 'p', 's', 'rt')}
        col['st'] = None if hs else op.get_vector('st', rhs=j)
        col.update(scalars=sc[:, [L.S_MU, L.S_DELTA, L.S_GAMMA, L.S_NU, L.S_RR]], alpha=cf[:, 0], beta=cf[:, 1], nu_pred=cf[:, 2],
                   hist=op.history(rhs=j)['updated_residual_2_norm'])
        cols.append(col)
    return cols, sched


KEYS = ('x', 'r', 'p', 's', 'rt', 'st', 'scalars', 'alpha', 'beta', 'nu_pred', 'hist')


def assert_column_bits(got, want, what, keys=KEYS):
    for q in keys:
        if want[q] is None:
            assert got[q] is None, (what, q)
            continue
        g, w = np.asarray(got[q]), np.asarray(want[q])
        assert g.shape == w.shape, (what, q, g.shape, w.shape)
        if not np.array_equal(g, w, equal_nan=True):
            bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))
            raise AssertionError(f'{what}: {q} differs in {len(bad)} of {g.size} entries, first at {bad[0]}: '
                                 f'got {g[tuple(bad[0])]!r} want {w[tuple(bad[0])]!r}')


def assert_finite_nonzero(want, what, hs):
    """every oracle inner product of every compared iteration is finite and nonzero (a case that breaks down is a wrong case)"""
    sc = want['scalars'][:, [0, 3, 4]] if hs else want['scalars']
    assert np.isfinite(sc).all() and (sc != 0).all(), f'{what}: an oracle inner product is zero or not finite'
    assert np.isfinite(want['x']).all(), what
