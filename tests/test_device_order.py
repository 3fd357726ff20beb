"""CPU: the model of the device's summation order (tests/device_order.py) on its own -- synthetic layouts, no GPU.

What tests/test_trajectory_oracle.py relies on: the tile tree sums every row exactly once in the order the kernel does
(OneLaunchTree), the pair-layout update-kernel tree (pair_sum), the XCD remap, the per-product routing (Routed) -- and that
ONE row summed twice, dropped or taken from a stale buffer at ONE iteration of a run hundreds of iterations long changes
the bits of that iteration's inner products (so a bit-for-bit comparison with the device sees it)."""
import math

import numpy as np
import pytest

from device_order import (OneLaunchTree, Routed, device_sum, first_mismatch, pair_dot, pair_sum, xcd_remap)
from oracle import ne_oracle as orc


def synthetic_layout(ntiles, rows_per_tile, grid, wpb, last_rows=None, first_row=0):
    """what DeviceCSR.layout() returns for `ntiles` consecutive tiles of rows_per_tile rows (the last one last_rows long)"""
    rb = first_row + rows_per_tile * np.arange(ntiles)
    re = rb + rows_per_tile
    if last_rows is not None:
        re[-1] = rb[-1] + last_rows
    return {'window': True, 'geometry': 0, 'rows_per_tile': rows_per_tile, 'tiles': np.stack([rb, re], axis=1), 'grid': grid,
            'waves_per_block': wpb, 'interior_tiles': ntiles, 'sweep_waves': 0}


def tiles_for(grid, wpb, shape):
    """tile counts that make the wave loop go wrong if it can: fewer tiles than waves, exactly three per wave, and a
    last round that only some waves take"""
    W = grid * wpb
    return {'fewer_than_waves': max(1, W - 3), 'three_per_wave': 3 * W, 'partial_round': 2 * W + max(1, W // 3)}[shape]


LAYOUTS = [(g, w, m, shape) for g in (1, 7, 8, 9, 235) for w in (2, 4, 16) for m in (64, 128)
           for shape in ('fewer_than_waves', 'three_per_wave', 'partial_round')]


def test_xcd_remap_is_a_permutation_for_every_grid():
    for nb in range(1, 301):
        assert sorted(xcd_remap(b, nb) for b in range(nb)) == list(range(nb)), nb
    # the remainder branch: workgroups b, b + 8, ... of one XCD get CONSECUTIVE positions, XCDs below nb % 8 one more
    assert [xcd_remap(b, 11) for b in range(11)] == [0, 2, 4, 6, 7, 8, 9, 10, 1, 3, 5]


@pytest.mark.parametrize('grid,wpb,rows,shape', LAYOUTS)
def test_tile_tree_on_synthetic_layouts(grid, wpb, rows, shape):
    """Every row once (the constructor asserts it), ragged last tile, a valid summation: within 1e-13 * sum|terms| of the
    exactly rounded sum (the bound test_oracle_golden.py holds device_dot to); np.float64 out."""
    nt = tiles_for(grid, wpb, shape)
    lay = synthetic_layout(nt, rows, grid, wpb, last_rows=rows - 39)
    tree = OneLaunchTree(lay)
    n = int(lay['tiles'][-1, 1])
    assert tree.idx.shape[:2] == (grid, wpb) and tree.idx.shape[2] == -(-nt // (grid * wpb)) * (rows // 64)
    if shape == 'fewer_than_waves':
        assert (tree.idx[:, :, 0, 0] < 0).sum() == grid * wpb - nt           # waves without a tile add nothing
    rng = np.random.default_rng(grid * 1000 + wpb * 10 + rows)
    prod = rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))
    got = tree.sum(prod)
    assert type(got) is np.float64
    assert abs(got - math.fsum(prod)) <= 1e-13 * math.fsum(np.abs(prod))
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    assert tree.dot(a, b) == tree.sum(a * b)
    # an exact case: integers sum without rounding in any order
    ints = rng.integers(-1000, 1000, n).astype(np.float64)
    assert tree.sum(ints) == ints.sum()


def test_tile_tree_order_within_and_across_lanes():
    """A lane adds its rows in sequence starting from +0.0: exchanging the FIRST TWO rows of one lane's column changes no bit
    (addition commutes); exchanging later ones re-associates the lane's sum, and moving a row to another lane re-associates
    the butterfly -- both stay valid summations and both can change bits, so the device's order has to be the model's."""
    lay = synthetic_layout(3 * 7 * 4, 128, 7, 4, last_rows=77)            # three 128-row tiles per wave: six rows per lane
    tree = OneLaunchTree(lay)
    n = int(lay['tiles'][-1, 1])
    rng = np.random.default_rng(5)
    bound = None
    changed_late = changed_lane = 0
    for trial in range(40):
        prod = rng.standard_normal(n)                                    # (like magnitudes: a re-association shows in the last bit)
        ref = tree.sum(prod)
        bound = 1e-13 * math.fsum(np.abs(prod))
        b, v, lane = rng.integers(7), rng.integers(4), rng.integers(64)
        col = tree.idx[b, v, :, lane]
        col = col[col >= 0]
        assert col.size >= 5
        p = prod.copy()
        p[[col[0], col[1]]] = p[[col[1], col[0]]]
        assert tree.sum(p) == ref                                        # first two of a column: bit-identical
        p = prod.copy()
        p[[col[1], col[4]]] = p[[col[4], col[1]]]
        got = tree.sum(p)
        assert abs(got - ref) <= 2 * bound
        changed_late += got != ref
        other = tree.idx[b, v, 0, (lane + 1 + rng.integers(63)) % 64]    # same wave, same step, another lane
        p = prod.copy()
        p[[col[0], other]] = p[[other, col[0]]]
        got = tree.sum(p)
        assert abs(got - ref) <= 2 * bound
        changed_lane += got != ref
    assert changed_late > 0 and changed_lane > 0, (changed_late, changed_lane)


def test_pair_layout_update_tree_is_a_valid_summation_and_not_the_pipelined_one():
    rng = np.random.default_rng(7)
    differs = 0
    for n in (1, 2, 3, 63, 64, 511, 512, 513, 729, 4097, 20_000, 1_200_001):
        a, b = rng.standard_normal(n), rng.standard_normal(n)
        got = pair_dot(a, b)
        assert type(got) is np.float64
        assert abs(got - math.fsum(a * b)) <= 1e-13 * math.fsum(np.abs(a * b))
        ints = rng.integers(-1000, 1000, n).astype(np.float64)
        assert pair_sum(ints) == ints.sum()
        differs += got != device_sum(a * b)
    assert differs > 0          # (thread t takes elements 2t, 2t + 1 here, t and t + 256 in k_pipe_update)
    # the order shows in the rounding: thread 1 adds its neighbours 2^-53 + 2^-53 = 2^-52 first, which survives beside the 1;
    # k_pipe_update's threads 2 and 3 hold one each, and 1 + 2^-53 rounds back to 1 twice
    x = np.zeros(1024)
    x[[0, 2, 3]] = [1.0, 2.0 ** -53, 2.0 ** -53]
    assert pair_sum(x) == 1.0 + 2.0 ** -52 and device_sum(x) == 1.0


def test_routed_dot_follows_the_call_order_and_survives_a_breakdown():
    seen = []
    r = Routed(lambda p: seen.append('nu') or p.sum(), lambda p: seen.append('mu') or p.sum())
    one = np.ones(4)
    for _ in range(3):
        r(one, one)
    assert seen == ['nu', 'mu', 'nu'] and r.calls == 3
    z = Routed(lambda p: 0.0)(one, one)
    assert type(z) is np.float64
    with np.errstate(all='ignore'):
        assert np.isinf(np.float64(1.0) / z) and np.isnan(z / z)         # a Python float would raise ZeroDivisionError
    tree = OneLaunchTree(synthetic_layout(2, 64, 1, 2))
    with np.errstate(all='ignore'):
        assert np.isnan(tree.dot(np.zeros(128), one[:1].repeat(128)) / tree.sum(np.zeros(128)))


class FaultyTree:
    """tree.sum with ONE fault at ONE call: a row summed twice, a row dropped, or a row's product taken from the array of
    the call two before (iteration k reading iteration k-2's buffer).  The row is the one with the largest term of that call: a
    term below the rounding of the sum cannot show in the sum whatever happens to it (the device tests hold x and r, too)."""

    def __init__(self, tree, kind, at_call):
        self.tree, self.kind, self.at, self.calls, self.seen = tree, kind, at_call, 0, []

    def sum(self, prod):
        prod = np.asarray(prod, dtype=np.float64)
        self.seen = (self.seen + [prod.copy()])[-3:]
        self.calls += 1
        if self.calls - 1 != self.at:
            return self.tree.sum(prod)
        p = prod.copy()
        row = int(np.argmax(np.abs(prod)))
        if self.kind == 'twice':
            p[row] = 2.0 * p[row]
        elif self.kind == 'dropped':
            p[row] = 0.0
        else:
            p[row] = self.seen[0][row]
        return self.tree.sum(p)


@pytest.mark.parametrize('kind', ['twice', 'dropped', 'stale'])
@pytest.mark.parametrize('method,prec,per_iter', [('hs_cg', False, 2), ('pr_pcg', True, 4), ('cg_cg', False, 2), ('pipe_pr_pcg', True, 4)])
def test_one_wrong_row_at_one_iteration_of_a_long_run_shows_in_the_bits(matrices, method, prec, per_iter, kind):
    """nos7 (n = 729) on a synthetic layout of twelve 64-row tiles (the last one 25 rows) on 2 workgroups of 4 waves: 400
    iterations with the tree, then again with one fault in one inner product of iteration 301.  The trajectories agree bit
    for bit up to iteration 300 and differ at 301 -- which is all a bit-for-bit comparison with the device needs."""
    A, z = matrices['nos7']
    n = A.shape[0]
    lay = synthetic_layout(12, 64, 2, 4, last_rows=n - 11 * 64)
    tree = OneLaunchTree(lay)
    kw = {'preconditioner': orc.jacobi(A)} if prec else {}
    iters, k_bad = 400, 301

    def run(t):
        rows = []
        getattr(orc, method)(A, z['b'], np.zeros(n), iters, dot=Routed(t.sum), dot0=pair_dot, square=lambda a: a * a,
                             tap=lambda st: rows.append((st.mu, st.dl, st.gm, st.nu, st.eta, st.alpha, st.beta)), **kw)
        return np.array(rows)

    clean = run(tree)
    assert np.isfinite(clean).all() and clean.shape == (iters, 7)
    # the second inner product of iteration k_bad
    faulty = run(FaultyTree(tree, kind, (k_bad - 1) * per_iter + 1))
    assert first_mismatch(faulty, clean) == k_bad, (first_mismatch(faulty, clean), k_bad)
    assert first_mismatch(clean, clean.copy()) == -1
    nan = clean.copy()
    nan[17, 2] = np.nan
    assert first_mismatch(nan, nan) == 17           # NaN never passes as equal
