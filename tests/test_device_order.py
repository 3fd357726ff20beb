"""CPU: the model of the device's summation order (tests/device_order.py) on its own -- synthetic layouts, no GPU.

What tests/test_trajectory_oracle.py relies on: the tile tree sums every row exactly once in the order the kernel does
(OneLaunchTree), the pair-layout update-kernel tree (pair_sum), the XCD remap, the per-product routing (Routed), the unit
tree of the sliced-row and CSR-adaptive launches (UnitTree: variable steps per unit, named rows, idle lanes) with the long-row
product of the CSR-adaptive tiles (LongRowOperator: what tests/test_trajectory_irregular.py relies on) -- and that ONE row summed twice, dropped or taken from a stale buffer at ONE iteration of a run hundreds of iterations long changes
the bits of that iteration's inner products (so a bit-for-bit comparison with the device sees it); likewise ONE wrong
application of a block-Jacobi preconditioner -- a stale u~, one block summed in another order -- which is what
tests/test_trajectory_stored_tilde.py is there to see.

What tests/test_trajectory_ranks.py relies on (the last section): the trees of ONE RANK of a multi-rank session -- the one-launch
iteration over the peer exchange (PeerLaunchTree: a communication wave, <= 8 boundary tiles relayed to it), a product in two
launches (TwoLaunchTree) -- and the rank-order sum (RankSum); and that ranks added in another order, a slot added twice, a
boundary tile's rows lost or a halo one iteration stale, at ONE iteration of a run, change the bits from there on.

What tests/test_trajectory_ranks_irregular.py relies on: the same product in two launches on sliced rows and CSR-adaptive tiles
(TwoLaunchUnitTree: each launch numbers the units of ITS class from 0, the partial rows lie interior first) against a slow
restatement, what it discriminates, and a ghost row of the PAIR array one iteration stale on one rank."""
import math

import numpy as np
import pytest
import scipy.sparse as sp

from device_order import (RELAY_TILES, LongRowOperator, OneLaunchTree, PeerLaunchTree, RankSum, Routed, TwoLaunchTree, TwoLaunchUnitTree, UnitTree,
                          device_sum, first_mismatch, long_row_sum, pair_dot, pair_sum, slice_units, tile_cap_nnz, tile_units, xcd_remap)
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


class FaultyBlockJacobi:
    """BlockJacobi with ONE fault at ONE application: 'stale' hands back what the application two before returned (in the
    pipelined flavours that recompute w: the u~ of the previous iteration, left in its buffer); 'reversed' sums the columns of
    ONE block in descending order -- the block with the largest result among those where the order shows in the bits."""

    def __init__(self, P, kind, at_call):
        self.P, self.kind, self.at, self.calls, self.seen, self.changed = P, kind, at_call, 0, [], 0

    def __call__(self, v):
        out = self.P(v)
        self.seen = (self.seen + [out.copy()])[-3:]
        self.calls += 1
        if self.calls - 1 != self.at:
            return out
        if self.kind == 'stale':
            self.changed = int(np.count_nonzero(self.seen[0] != out))
            return self.seen[0].copy()
        bs, B = self.P.bs, self.P.inv_blocks
        nf = out.shape[0] // bs
        V = np.asarray(v, dtype=np.float64)[:nf * bs].reshape(nf, bs)
        rev = B[:nf, :, bs - 1] * V[:, bs - 1:bs]
        for j in range(bs - 2, -1, -1):
            rev = rev + B[:nf, :, j] * V[:, j:j + 1]
        fwd = out[:nf * bs].reshape(nf, bs)
        shows = (rev != fwd).any(axis=1)
        assert shows.any()
        k = int(np.argmax(np.where(shows, np.abs(fwd).max(axis=1), -1.0)))
        self.changed = int(np.count_nonzero(rev[k] != fwd[k]))
        out = out.copy()
        out[k * bs:(k + 1) * bs] = rev[k]
        return out


@pytest.mark.parametrize('kind', ['stale', 'reversed'])
def test_one_wrong_application_of_block_jacobi_in_a_long_run_shows_in_the_bits(matrices, kind):
    """What tests/test_trajectory_stored_tilde.py is for, on the model's side: pipe_pr_pcg on bcsstk03 (n = 112) under
    BlockJacobi(A, 8) with the sums of that schedule (the pipelined update tree for every inner product), 90 iterations --
    below the oracle's first non-positive nu at k = 128 --, then again with one fault in the u~ that iteration 50 uses
    (M^-1 is applied to r, s, u at the start and to u, then w, in every iteration: application 3 + 2 (50 - 2)).  The trajectories
    agree bit for bit before iteration 50.  A stale u~ (all 112 entries of another iteration) differs at 50: u~ enters s~ =
    (w~ - a u~) + b s~ there, hence delta and gamma.  One block summed in reverse order changes the last bit of at most 8
    entries of u~, which may stay below the rounding of those two 112-term sums; s~ of iteration 50 carries it into r~, p, s and
    u of 51 and into every inner product by 52 -- the first difference lies in 50..52.  From the first difference on every
    iteration differs, the last one included."""
    import new_cg_variants_amd.cg_variants as cgv
    from device_order import device_dot
    A, z = matrices['bcsstk03']
    n = A.shape[0]
    P = cgv.BlockJacobi(A, 8)
    iters, k_bad = 90, 50

    def run(M):
        rows = []
        orc.pipe_pr_pcg(A, z['b'], np.zeros(n), iters, preconditioner=M, dot=device_dot, dot0=device_dot, square=lambda a: a * a,
                        tap=lambda st: rows.append((st.mu, st.dl, st.gm, st.nu, st.eta, st.alpha, st.beta)))
        return np.array(rows)

    clean = run(P)
    assert np.isfinite(clean).all() and clean.shape == (iters, 7) and (clean[:, [0, 1, 2, 3]] != 0).all()
    assert first_mismatch(run(FaultyBlockJacobi(P, kind, -1)), clean) == -1          # the wrapper alone changes nothing
    M = FaultyBlockJacobi(P, kind, 3 + 2 * (k_bad - 2))
    faulty = run(M)
    assert M.calls == 3 + 2 * (iters - 1)
    first = first_mismatch(faulty, clean)
    if kind == 'stale':
        assert M.changed == n and first == k_bad, (M.changed, first)
    else:
        assert 1 <= M.changed <= 8 and k_bad <= first <= k_bad + 2, (M.changed, first)
    differs = (faulty != clean).any(axis=1)
    assert differs[first:].all() and differs[-1] and not differs[:first].any()


# ---- UnitTree: sliced rows and CSR-adaptive tiles (tests/test_trajectory_irregular.py) ------------------------------------
def unit_layout(grid, tiles=None, slice_rows=None):
    """what DeviceCSR.layout() returns for a CSR-adaptive operator (tiles) or a sliced-row operator (slice_rows)"""
    sliced = slice_rows is not None
    return {'window': False, 'geometry': -1, 'rows_per_tile': 0, 'grid': grid, 'waves_per_block': 4, 'interior_tiles': 0, 'sweep_waves': 0,
            'tiles': np.zeros((0, 2), dtype=np.int64) if tiles is None else np.asarray(tiles, dtype=np.int64), 'sliced': sliced,
            'slice_rows': np.asarray(slice_rows, dtype=np.int32).reshape(-1, 64) if sliced else np.zeros((0, 64), dtype=np.int32)}


def tiles_of(sizes):
    re = np.cumsum(sizes)
    return np.stack([re - sizes, re], axis=1)


def synthetic_units(kind, count, rng):
    """a layout's unit table with `count` units.  'tiles': CSR-adaptive tiles of 1..256 rows with 63, 64, 65, 129, 256 and a
    one-row tile among them; 'full': full slices and a ragged last one; 'cut': slices of 1..64 consecutive rows (the idle lanes
    behind); 'named': sorting windows of four slices whose rows are named in a permuted order, the idle lanes of a window in the
    middle of its last slice's lanes"""
    if kind == 'tiles':
        sizes = rng.integers(1, 257, count)
        special = [63, 64, 65, 129, 256, 1]
        sizes[rng.permutation(count)[:min(count, len(special))]] = special[:min(count, len(special))]
        return {'tiles': tiles_of(sizes)}
    lane = np.arange(64)
    if kind == 'full':
        rows = 64 * np.arange(count)[:, None] + lane[None, :]
        rows[-1, 25:] = -1
        return {'slice_rows': rows}
    if kind == 'cut':
        t = tiles_of(rng.integers(1, 65, count))
        rows = t[:, :1] + lane[None, :]
        return {'slice_rows': np.where(rows < t[:, 1:], rows, -1)}
    out, first = [], 0
    for w in range(0, count, 4):
        ns = min(4, count - w)
        nrows = 64 * ns - int(rng.integers(0, 40))
        win = -np.ones(64 * ns, dtype=np.int64)
        keep = np.sort(rng.permutation(64 * ns)[:nrows])             # (idle lanes anywhere in the window)
        win[keep] = first + rng.permutation(nrows)
        out.append(win.reshape(ns, 64))
        first += nrows
    return {'slice_rows': np.concatenate(out)}


UNIT_CASES = [(g, kind, shape) for g in (1, 7, 8, 9, 143) for kind in ('tiles', 'full', 'cut', 'named')
              for shape in ('fewer_than_waves', 'three_per_wave', 'partial_round')]


@pytest.mark.parametrize('grid,kind,shape', UNIT_CASES)
def test_unit_tree_on_synthetic_units(grid, kind, shape):
    """Every row once (the constructor asserts it), whatever the unit: a valid summation within 1e-13 * sum|terms| of the
    exactly rounded sum, np.float64 out, exact on integers; a wave's steps are the steps of its units one after the other."""
    count = tiles_for(grid, 4, shape)
    rng = np.random.default_rng(grid * 100 + len(kind) * 10 + len(shape))
    lay = unit_layout(grid, **synthetic_units(kind, count, rng))
    tree = UnitTree.of(lay)
    assert tree.idx.shape[:2] == (grid, 4) and tree.idx.shape[3] == 64
    n = tree.rows[1]
    assert tree.rows[0] == 0 and np.count_nonzero(tree.idx >= 0) == n
    if kind == 'tiles':
        steps = -(-(lay['tiles'][:, 1] - lay['tiles'][:, 0]) // 64)
        per_wave = [sum(steps[xcd_remap(b, grid) * 4 + v::grid * 4]) for b in range(grid) for v in range(4)]
        assert tree.idx.shape[2] == max(per_wave)
        sizes = lay['tiles'][:, 1] - lay['tiles'][:, 0]
        assert count < 6 or {1, 63, 64, 65, 129, 256} <= set(sizes.tolist())
        for one in np.flatnonzero(sizes == 1):                 # a one-row tile: lane 0 alone
            where = np.argwhere(tree.idx == lay['tiles'][one, 0])
            assert where.shape == (1, 4) and where[0, 3] == 0
            b, v, st = where[0, :3]
            assert (tree.idx[b, v, st, 1:] == -1).all()
    else:
        assert tree.idx.shape[2] == -(-count // (grid * 4))
    if shape == 'fewer_than_waves':
        assert (tree.idx[:, :, 0, :] < 0).all(axis=2).sum() == grid * 4 - count          # waves without a unit add nothing
    prod = rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))
    got = tree.sum(prod)
    assert type(got) is np.float64
    assert abs(got - math.fsum(prod)) <= 1e-13 * math.fsum(np.abs(prod))
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    assert tree.dot(a, b) == tree.sum(a * b)
    ints = rng.integers(-1000, 1000, n).astype(np.float64)
    assert tree.sum(ints) == ints.sum()


def test_unit_tree_refuses_a_row_summed_twice_or_never():
    rows = 64 * np.arange(5)[:, None] + np.arange(64)[None, :]
    UnitTree.of(unit_layout(2, slice_rows=rows))
    twice = rows.copy()
    twice[3] = twice[2]
    with pytest.raises(AssertionError, match='exactly once'):
        UnitTree.of(unit_layout(2, slice_rows=twice))
    with pytest.raises(AssertionError, match='exactly once'):
        UnitTree.of(unit_layout(2, slice_rows=np.delete(rows, 2, axis=0)))
    with pytest.raises(AssertionError, match='exactly once'):
        UnitTree.of(unit_layout(2, tiles=[[0, 100], [90, 200]]))


@pytest.mark.parametrize('grid,wpb,rows,shape', [c for c in LAYOUTS if c[0] in (7, 9) or c[1] == 4])
def test_unit_tree_built_like_a_window_layout_gives_the_bits_of_the_tile_tree(grid, wpb, rows, shape):
    nt = tiles_for(grid, wpb, shape)
    lay = synthetic_layout(nt, rows, grid, wpb, last_rows=rows - 39)
    lane = np.arange(64)
    units = []
    for rb, re in lay['tiles']:
        r = rb + 64 * np.arange(rows // 64)[:, None] + lane[None, :]
        units.append(np.where(r < re, r, -1))                 # (a window tile has rows_per_tile / 64 steps, idle or not)
    unit, tile = UnitTree(units, grid, wpb), OneLaunchTree(lay)
    assert np.array_equal(unit.idx, tile.idx)
    rng = np.random.default_rng(grid + wpb + rows)
    for _ in range(3):
        prod = rng.standard_normal(int(lay['tiles'][-1, 1]))
        assert unit.sum(prod) == tile.sum(prod)


def test_unit_tree_discriminates():
    """What the device's order could differ in without losing a row -- each changes bits of the sum of a fixed random vector
    (three vectors: 'at least one bit' of any of the three sums), so the bit-for-bit comparison with the device sees it."""
    rng = np.random.default_rng(2024)
    grid = 9
    named = synthetic_units('named', 3 * grid * 4, rng)['slice_rows']
    n = int(named.max()) + 1
    vecs = [rng.standard_normal(n) for _ in range(3)]

    def sums(tree, vecs=vecs):
        assert tree.rows == (0, vecs[0].shape[0])
        return [tree.sum(v) for v in vecs]
    ref = sums(UnitTree.of(unit_layout(grid, slice_rows=named)))
    # two slices exchanged between two waves of one workgroup
    swapped = named.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    assert sums(UnitTree.of(unit_layout(grid, slice_rows=swapped))) != ref
    # the same slice table, the rows taken as consecutive instead of as named
    flat = -np.ones_like(named)
    flat[named >= 0] = np.arange(n)
    assert np.array_equal(flat >= 0, named >= 0)
    assert sums(UnitTree.of(unit_layout(grid, slice_rows=flat))) != ref
    # a 65-row tile: two steps of ONE wave (row 64 joins lane 0's accumulator) -- not a unit of 64 rows and a unit of one
    sizes = np.full(3 * grid * 4, 64)
    sizes[5] = 65
    t = tiles_of(sizes)
    vecs_t = [rng.standard_normal(int(t[-1, 1])) for _ in range(3)]
    ref_t = sums(UnitTree.of(unit_layout(grid, tiles=t)), vecs_t)
    split = np.concatenate([t[:5], [[t[5, 0], t[5, 0] + 64], [t[5, 0] + 64, t[5, 1]]], t[6:]])
    assert sums(UnitTree.of(unit_layout(grid, tiles=split)), vecs_t) != ref_t
    # a long row: 64 lane sums and the butterfly, not left to right
    long = [rng.standard_normal(2500) for _ in range(3)]
    left = []
    for p in long:
        s = 0.0
        for x in p:
            s += x
        left.append(s)
    assert [long_row_sum(p) for p in long] != left
    assert all(abs(long_row_sum(p) - math.fsum(p)) <= 1e-14 * math.fsum(np.abs(p)) for p in long)


def long_row_matrix(rng, n, long_rows):
    """random sparse rows of 3..40 entries, the rows in `long_rows` (row -> entries) long, a dominant diagonal"""
    lens = rng.integers(3, 41, n)
    for i, m in long_rows.items():
        lens[i] = m
    indptr = np.concatenate([[0], np.cumsum(lens)])
    indices = np.concatenate([np.sort(rng.permutation(n)[:m]) for m in lens])
    A = sp.csr_matrix((rng.standard_normal(indptr[-1]) * np.exp(rng.uniform(-3, 3, indptr[-1])), indices, indptr), shape=(n, n))
    return A


def test_long_row_operator():
    """SciPy's product bit for bit while no row exceeds the cap; with long rows within DESIGN.md's bar for them, 1e-14 * sum|a_ij x_j|
    per row, and NOT SciPy's bits; shape and diagonal forwarded; the cap of schedule()['tile_steps']."""
    assert [tile_cap_nnz(s) for s in (1, 2, 4)] == [253, 509, 1021]
    rng = np.random.default_rng(11)
    n = 3000
    A = long_row_matrix(rng, n, {7: 509, 1200: 2000, 2999: 2600, 40: 510})
    x = rng.standard_normal(n)
    plain = LongRowOperator(A, 2600)
    assert plain.long_rows.size == 0 and np.array_equal(plain @ x, A @ x)
    op = LongRowOperator(A, tile_cap_nnz(2))
    assert list(op.long_rows) == [40, 1200, 2999]                # (a row of exactly the cap is no long row)
    assert op.shape == A.shape and np.array_equal(op.diagonal(), A.diagonal())
    got, want = op @ x, A @ x
    short = np.setdiff1d(np.arange(n), op.long_rows)
    assert np.array_equal(got[short], want[short])
    bound = 1e-14 * (abs(A) @ np.abs(x))
    assert (np.abs(got - want) <= bound).all()
    assert np.count_nonzero(got != want) >= 1
    assert (got[[1200, 2999]] != want[[1200, 2999]]).any()       # a row of >= 2000 entries shows the other order
    for i in op.long_rows:
        lo, hi = A.indptr[i], A.indptr[i + 1]
        terms = A.data[lo:hi] * x[A.indices[lo:hi]]
        assert abs(got[i] - math.fsum(terms)) <= 1e-14 * math.fsum(np.abs(terms))
        # the model of the lanes: lane l sums terms l, l + 64, ... left to right
        lanes = []
        for l in range(64):
            s = 0.0
            for t in terms[l::64]:
                s += t
            lanes.append(s)
        v = np.array(lanes)
        for off in (32, 16, 8, 4, 2, 1):
            v = v + v[np.arange(64) ^ off]                       # the xor butterfly itself, every lane
        assert (v == v[0]).all() and got[i] == v[0]


# ---- several ranks: PeerLaunchTree, TwoLaunchTree, RankSum (tests/test_trajectory_ranks.py) -------------------------------------
def rank_layout(ntiles, nbnd, grid, wpb, rows_per_tile=64, last_rows=None):
    """what DeviceCSR.layout() returns for one rank of a row-block run: `ntiles` consecutive tiles of the rank's local rows, the
    nbnd tiles next to the cuts (half of them at the block's first rows, the others at its last) BEHIND the interior ones in the
    table, as the planner orders them; the block's last tile `last_rows` long"""
    rb = rows_per_tile * np.arange(ntiles)
    re = rb + rows_per_tile
    if last_rows is not None:
        re[-1] = rb[-1] + last_rows
    lo = nbnd // 2
    order = list(range(lo, ntiles - (nbnd - lo))) + list(range(lo)) + list(range(ntiles - (nbnd - lo), ntiles))
    return {'window': True, 'geometry': 0, 'rows_per_tile': rows_per_tile, 'tiles': np.stack([rb, re], axis=1)[order], 'grid': grid,
            'waves_per_block': wpb, 'interior_tiles': ntiles - nbnd, 'sweep_waves': 0, 'interior_grid': 0, 'interior_waves_per_block': 0}


def as_two_launches(lay):
    """the same rank after an overlapped product: the interior launch keeps the shape, the boundary launch has one wave per tile"""
    nb = lay['tiles'].shape[0] - lay['interior_tiles']
    return dict(lay, interior_grid=lay['grid'], interior_waves_per_block=lay['waves_per_block'], grid=-(-nb // lay['waves_per_block']))


BOUNDARY = (0, 3, RELAY_TILES, RELAY_TILES + 1)            # both sides of kRelayTiles, and a rank that reads no ghost rows


@pytest.mark.parametrize('wpb', [4, 8])
@pytest.mark.parametrize('grid', [1, 8, 9, 256])
@pytest.mark.parametrize('nranks', [2, 3, 4])
def test_rank_trees_on_synthetic_layouts(nranks, grid, wpb):
    """Ranks with 0, 3, 8 and 9 boundary tiles (which of them: shifted by the case) on `grid` workgroups of `wpb` waves; rank 1 has
    fewer tiles than waves, the others a last round that only some waves take.  Every tree sums every row of its rank once (the
    constructors assert it) and the rank-order sum of each kind of tree is a valid summation: within 1e-13 * sum|terms| of the
    exactly rounded sum, exact on integers, np.float64 out."""
    W = grid * wpb
    rng = np.random.default_rng(nranks * 10000 + grid * 10 + wpb)
    lays = []
    for r in range(nranks):
        nbnd = BOUNDARY[(r + grid + wpb // 4) % 4]
        nt = max(nbnd + 1, W - 3) if r == 1 else 2 * W + max(1, W // 3)
        lays.append(rank_layout(nt, nbnd, grid, wpb, last_rows=25))
    assert lays[1]['tiles'].shape[0] < W or W <= RELAY_TILES + 4
    offsets = np.concatenate([[0], np.cumsum([int(l['tiles'][:, 1].max()) for l in lays])])
    peer = [PeerLaunchTree(l) for l in lays]
    plain = [OneLaunchTree(l) for l in lays]
    for l, t, o in zip(lays, peer, plain):
        nb = l['tiles'].shape[0] - l['interior_tiles']
        assert t.relayed == (0 < nb <= RELAY_TILES)
        assert np.array_equal(np.sort(t.idx[t.idx >= 0]), np.sort(o.idx[o.idx >= 0]))          # the same rows, each once
        s0 = [(b, v) for b in range(grid) for v in range(wpb) if xcd_remap(b, grid) * wpb + v == 0]
        assert s0 == [(0, 0)]
        comm = t.idx[0, 0]
        # the communication wave: the boundary tiles one after another when it relays them, else nothing
        want = np.concatenate([np.arange(rb, re) for rb, re in l['tiles'][l['interior_tiles']:]]) if t.relayed else np.zeros(0)
        assert np.array_equal(np.sort(comm[comm >= 0]), np.sort(want))
    kinds = {'peer': [t.sum for t in peer], 'gather': [t.sum for t in plain],
             'two launches': [TwoLaunchTree(as_two_launches(l)).sum if 0 < l['interior_tiles'] < l['tiles'].shape[0] else pair_sum for l in lays],
             'mixed': [(peer[r].sum, device_sum, pair_sum, plain[r].sum)[r] for r in range(nranks)]}
    n = int(offsets[-1])
    prod = rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))
    ints = rng.integers(-1000, 1000, n).astype(np.float64)
    for kind, sums in kinds.items():
        rs = RankSum(offsets, sums)
        got = rs(prod)
        assert type(got) is np.float64, kind
        assert abs(got - math.fsum(prod)) <= 1e-13 * math.fsum(np.abs(prod)), kind
        assert rs(ints) == ints.sum(), kind
        a = rng.standard_normal(n)
        assert rs.dot(a, prod) == rs(a * prod)
        slots = rs.slots(prod)
        want = slots[0]
        for v in slots[1:]:
            want = want + v
        assert len(slots) == nranks and got == want, kind


def test_peer_tree_assignment_and_its_difference_from_the_plain_one():
    """The assignment on a layout small enough to write down, both sides of kRelayTiles; a launch of one workgroup of two
    waves; and on a rank WITHOUT boundary tiles the peer tree covers the rows of OneLaunchTree and differs from it in bits (every
    wave's tiles are shifted by one slot and stride W - 1)."""
    def tiles_of_wave(tree, lay, b, v):
        col = tree.idx[b, v, :, 0]
        first = {int(rb): i for i, (rb, re) in enumerate(lay['tiles'])}
        return [first[int(x)] for x in col[col >= 0] if int(x) in first]
    lay = rank_layout(7, 2, 1, 4)                               # table: interior tiles 0..4, boundary tiles 5, 6
    t = PeerLaunchTree(lay)
    assert t.relayed and [tiles_of_wave(t, lay, 0, v) for v in range(4)] == [[5, 6], [0, 3], [1, 4], [2]]
    lay = rank_layout(14, 9, 1, 4)                              # nine boundary tiles: they stay with all the waves
    t = PeerLaunchTree(lay)
    assert not t.relayed and [tiles_of_wave(t, lay, 0, v) for v in range(4)] == [[], [0, 3, 6, 9, 12], [1, 4, 7, 10, 13], [2, 5, 8, 11]]
    lay = rank_layout(3, 1, 1, 2)
    assert [tiles_of_wave(PeerLaunchTree(lay), lay, 0, v) for v in range(2)] == [[2], [0, 1]]
    with pytest.raises(AssertionError, match='exactly once'):
        PeerLaunchTree(dict(lay, tiles=lay['tiles'][[0, 1, 1]]))
    lay = rank_layout(3 * 9 * 4, 0, 9, 4, last_rows=25)
    peer, plain = PeerLaunchTree(lay), OneLaunchTree(lay)
    assert not peer.relayed and (peer.idx[0, 0] < 0).all()
    assert np.array_equal(np.sort(peer.idx[peer.idx >= 0]), np.sort(plain.idx[plain.idx >= 0]))
    rng = np.random.default_rng(3)
    vecs = [rng.standard_normal(int(lay['tiles'][:, 1].max())) for _ in range(3)]
    assert [peer.sum(v) for v in vecs] != [plain.sum(v) for v in vecs]
    assert all(abs(peer.sum(v) - plain.sum(v)) <= 2e-13 * math.fsum(np.abs(v)) for v in vecs)


def test_rank_sum_starts_from_rank_zero():
    """v = s[0]; v += s[r]: a sum that started from +0.0 would turn a first slot of -0.0 into +0.0"""
    rs = RankSum([0, 2, 4], [lambda p: np.float64(-0.0), lambda p: np.float64(-0.0)])
    assert np.signbit(rs(np.zeros(4)))
    order = []
    rs = RankSum([0, 1, 3, 6], [lambda p, r=r: order.append((r, p.shape[0])) or p.sum() for r in range(3)])
    assert rs(np.arange(6.0)) == 15.0 and order == [(0, 1), (1, 2), (2, 3)]
    big = RankSum([0, 1, 2, 3], [lambda p: p[0]] * 3)
    assert big(np.array([1.0, 2.0 ** -53, 2.0 ** -53])) == 1.0 and big(np.array([2.0 ** -53, 2.0 ** -53, 1.0])) == 1.0 + 2.0 ** -52


class StaleHaloOperator:
    """A as `nranks` row blocks multiply it, ONE product (call `at`, counted from 0) reading its GHOST columns -- the columns
    outside the rank's own rows -- from the vector of the call two before (the same product of the previous iteration: a halo one
    iteration stale).  Every row is still SciPy's left-to-right sum: only the values of the ghost entries differ.  span=2: that
    call and the next (both columns of a pair array: u = A s~ and w = A r~ of one pipelined iteration, each from ITS vector of the
    iteration before); ranks: only these ranks read stale ghost rows (None: all)."""

    def __init__(self, A, offsets, at, span=1, ranks=None):
        self.A, self.offsets, self.at, self.calls, self.seen, self.changed = A.tocsr(), [int(o) for o in offsets], at, 0, [], 0
        self.span, self.ranks = span, ranks
        self.shape = A.shape

    def diagonal(self):
        return self.A.diagonal()

    def __matmul__(self, v):
        v = np.asarray(v, dtype=np.float64)
        self.seen = (self.seen + [v.copy()])[-3:]
        self.calls += 1
        y = self.A @ v
        if self.at < 0 or not self.at <= self.calls - 1 < self.at + self.span:
            return y
        stale = self.seen[0]
        for q, (lo, hi) in enumerate(zip(self.offsets, self.offsets[1:])):
            if self.ranks is not None and q not in self.ranks:
                continue
            mixed = stale.copy()
            mixed[lo:hi] = v[lo:hi]
            y[lo:hi] = self.A[lo:hi] @ mixed
        self.changed += int(np.count_nonzero(y != self.A @ v))
        return y


class FaultyRankSum(RankSum):
    """RankSum with ONE fault in every inner product of ONE iteration (calls 4 (k - 1) .. 4 (k - 1) + 3 of pipe_pr_pcg's advance):
    'reversed' adds the ranks from the last to the first -- FROM that iteration on, as a rank with the wrong order would: most sums
    of a few slots of like size have the same bits in either order --, 'twice' adds rank 1's slot twice, 'tile_dropped' leaves the rows of
    rank 1's first boundary tile out of its sum."""

    def __init__(self, offsets, sums, kind, k_bad, drop_rows=None):
        super().__init__(offsets, sums)
        self.kind, self.k_bad, self.calls, self.drop_rows = kind, k_bad, 0, drop_rows

    def __call__(self, prod):
        k = self.calls // 4 + 1
        self.calls += 1
        if self.kind is None or k < self.k_bad or (k > self.k_bad and self.kind != 'reversed'):
            return super().__call__(prod)
        if self.kind == 'tile_dropped':
            p = np.array(prod, dtype=np.float64)
            p[self.drop_rows] = 0.0
            return super().__call__(p)
        s = self.slots(prod)
        if self.kind == 'reversed':
            s = s[::-1]
        v = s[0]
        for r in range(1, len(s)):
            v = v + s[r]
        return np.float64(v + s[1]) if self.kind == 'twice' else np.float64(v)


@pytest.mark.parametrize('kind,nranks', [('reversed', 4), ('twice', 2), ('tile_dropped', 2), ('stale_halo', 2), ('stale_pair_halo', 2)])
def test_one_wrong_exchange_at_one_iteration_of_a_multi_rank_run_shows_in_the_bits(kind, nranks):
    """What tests/test_trajectory_ranks.py is for, on the model's side: pipe_pr_pcg with Jacobi on a small band (the 5-point stencil
    on a 7 x 430 grid: n = 3010, 7-row halo, still converging at iteration 60 -- on the ex2b band Jacobi is the inverse to rounding,
    the run sits in a two-cycle of rounding noise from iteration 6 on and a wrong bit heals) in `nranks` row blocks, every rank on 4 workgroups of 4 waves with the peer tree (the boundary tiles next to the cuts
    relayed to the communication wave), the ranks added in rank order; 90 iterations, then again with one fault at iteration 50.
    Two ranks, except for the reversed order: s[0] + s[1] = s[1] + s[0] bit for bit, an order shows from three ranks on -- and
    even then it leaves most sums' bits alone (7 of 8 tried with three slots of like size), so that fault runs on four ranks and
    stays in force from iteration 50 on: it must show by iteration 52 like the stale halo.  The
    trajectories agree bit for bit before iteration 50 and differ from 50 (a wrong sum: that iteration's inner products), or
    within the next two iterations (a stale halo reaches u of iteration 50, w and s of 51 and every inner product by 52), and
    at every iteration after the first difference.  'stale_pair_halo' (tests/test_trajectory_ranks_irregular.py: the two launches of
    pipe_spmm_and_reduce read the ghost rows of the pair array (r~, s~) behind the rank's own pairs): BOTH products of iteration 50
    read their ghost columns one iteration stale, on rank 1 only -- at most its 7 ghost rows' neighbours change, per product."""
    from new_cg_variants_amd import problems
    iters, k_bad = 90, 50
    A = problems.laplace_2d(7, 430)
    n = A.shape[0]
    b, x0, _ = problems.reference_rhs(A, n)
    # (uneven blocks: the problem is symmetric under a reversal of the rows, and so would the outer ranks' sums be)
    offsets = np.round(n * np.array({2: [0, 0.43, 1], 4: [0, 0.19, 0.4, 0.73, 1]}[nranks])).astype(np.int64)
    lays = []
    for r in range(nranks):
        nt = -(-int(offsets[r + 1] - offsets[r]) // 64)
        nbnd = (r > 0) + (r < nranks - 1)
        lay = rank_layout(nt, nbnd, 4, 4, last_rows=int(offsets[r + 1] - offsets[r]) - 64 * (nt - 1))
        lays.append(lay)
    trees = [PeerLaunchTree(l) for l in lays]
    assert all(t.relayed for t in trees)
    rb, re = lays[1]['tiles'][lays[1]['interior_tiles']]
    drop = np.arange(offsets[1] + rb, offsets[1] + re)

    def run(fault, op=A):
        rows = []
        dot = FaultyRankSum(offsets, [t.sum for t in trees], fault, k_bad, drop)
        orc.pipe_pr_pcg(op, b, x0, iters, preconditioner=orc.jacobi(A), dot=Routed(dot), dot0=Routed(RankSum(offsets, [device_sum] * nranks)),
                        square=lambda a: a * a, tap=lambda st: rows.append((st.mu, st.dl, st.gm, st.nu, st.eta, st.alpha, st.beta)))
        assert dot.calls == 4 * (iters - 1)
        return np.array(rows)

    clean = run(None)
    assert np.isfinite(clean).all() and clean.shape == (iters, 7) and (clean[:, [0, 1, 2, 3]] > 0).all()
    if kind in ('stale_halo', 'stale_pair_halo'):
        pair = kind == 'stale_pair_halo'
        assert first_mismatch(run(None, StaleHaloOperator(A, offsets, -1)), clean) == -1       # the wrapper alone changes nothing
        # three products at the start, then u = A s~, w = A r~ per iteration
        op = StaleHaloOperator(A, offsets, 3 + 2 * (k_bad - 1), span=2 if pair else 1, ranks=(1,) if pair else None)
        faulty = run(None, op)
        assert op.calls == 3 + 2 * (iters - 1) and 1 <= op.changed <= 14 * (nranks - 1), op.changed
        lo, hi = k_bad, k_bad + 2
    else:
        faulty = run(kind)
        lo, hi = k_bad, k_bad + (2 if kind == 'reversed' else 0)
    first = first_mismatch(faulty, clean)
    assert lo <= first <= hi, (kind, first)
    differs = (faulty != clean).any(axis=1)
    assert differs[first:].all() and differs[-1] and not differs[:first].any()


# ---- a product in two launches on sliced rows and CSR-adaptive tiles: TwoLaunchUnitTree (tests/test_trajectory_ranks_irregular.py) ----
def rank_unit_layout(kind, n_int, n_bnd, g1, g2, rng):
    """what DeviceCSR.layout() returns for one rank after an overlapped product on `kind` units (synthetic_units), n_int interior
    ones on g1 workgroups in front of n_bnd boundary ones on g2; g1 == 0: one class is empty and the other ran alone on g2"""
    lay = unit_layout(g2, **synthetic_units(kind, n_int + n_bnd, rng))
    return dict(lay, interior_grid=g1, interior_waves_per_block=4 if g1 else 0, interior_tiles=0 if lay['sliced'] else n_int,
                interior_slices=n_int if lay['sliced'] else 0)


def slow_two_launch_sum(lay, prod):
    """TwoLaunchUnitTree.sum restated with scalars and loops, nothing shared with tests/device_order.py: the XCD order as "the
    workgroups of XCD 0 (b % 8 == 0) in launch order, then XCD 1's, ...", every lane's accumulator a Python float from +0.0"""
    if lay['sliced']:
        units = [[[int(r) for r in rows]] for rows in lay['slice_rows']]
        n_int = lay['interior_slices']
    else:
        units = [[[rb + 64 * j + l if rb + 64 * j + l < re else -1 for l in range(64)] for j in range(-(-(re - rb) // 64))] for rb, re in lay['tiles'].tolist()]
        n_int = lay['interior_tiles']
    launches = [(0, len(units), lay['grid'])] if lay['interior_grid'] == 0 else [(0, n_int, lay['interior_grid']), (n_int, len(units), lay['grid'])]

    def wave_sum(lanes):
        for off in (32, 16, 8, 4, 2, 1):
            lanes = [lanes[l] + lanes[l ^ off] for l in range(64)]
        return lanes[0]
    rows_of_partials = []
    for first, end, grid in launches:
        order = sorted(range(grid), key=lambda b: (b % 8, b // 8))
        for b in range(grid):
            waves = []
            for v in range(4):
                acc = [0.0] * 64
                u = first + order.index(b) * 4 + v
                while u < end:
                    for step in units[u]:
                        for l in range(64):
                            if step[l] >= 0:
                                acc[l] = acc[l] + float(prod[step[l]])
                    u += grid * 4
                waves.append(wave_sum(acc))
            rows_of_partials.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
    threads = [0.0] * 256
    for i, p in enumerate(rows_of_partials):
        threads[i % 256] = threads[i % 256] + p                         # (thread t: partials t, t + 256, ... in that order)
    w = [wave_sum(threads[64 * i:64 * i + 64]) for i in range(4)]
    return ((w[0] + w[1]) + w[2]) + w[3]


# (kind, interior units, boundary units, interior workgroups, boundary workgroups)
TWO_LAUNCH_CASES = [
    ('full', 34, 7, 9, 2),            # the shape of a 2-rank FEM block: a quarter of each class's units, the last slice ragged
    ('cut', 35, 13, 9, 4),            # idle lanes; 35 units on 36 waves, 13 on 16: waves without a unit in both launches
    ('named', 40, 24, 3, 2),          # named rows; 3 to 4 units per wave
    ('tiles', 150, 33, 38, 9),        # ragged tiles, several rows per lane
    ('tiles', 300, 290, 7, 70),       # more than 256 partial rows under the final tree: 77 + ... no -- 7 + 70; several rounds per wave
    ('tiles', 1100, 70, 260, 18),     # 278 partial rows: thread t of the final tree adds rows t and t + 256, across the two launches
    ('cut', 0, 14, 0, 4),             # no interior unit (g1 == 0): the boundary launch alone
    ('tiles', 0, 361, 0, 91),
    ('full', 41, 0, 0, 11),           # no boundary unit: the interior launch alone, reported as 'grid'
]


@pytest.mark.parametrize('kind,n_int,n_bnd,g1,g2', TWO_LAUNCH_CASES)
def test_two_launch_unit_tree_against_a_slow_restatement(kind, n_int, n_bnd, g1, g2):
    """Every row once over both launches (the constructor asserts it), the bits of the slow restatement on three vectors, a valid
    summation (1e-13 * sum|terms| of the exactly rounded sum), exact on integers, np.float64 out; partials() are the g1 + g2 rows
    and sum() their final tree; with one class empty the tree is UnitTree over the other class."""
    rng = np.random.default_rng(1000 * n_int + 10 * n_bnd + g1)
    lay = rank_unit_layout(kind, n_int, n_bnd, g1, g2, rng)
    tree = TwoLaunchUnitTree(lay)
    n = tree.rows[1]
    assert tree.rows[0] == 0 and (tree.interior_units, tree.units) == (n_int, n_int + n_bnd)
    assert len(tree.launches) == (2 if g1 else 1) and [l.grid for l in tree.launches] == ([g1, g2] if g1 else [g2])
    for _ in range(3):
        prod = rng.standard_normal(n) * np.exp(rng.uniform(-8, 8, n))
        got = tree.sum(prod)
        assert type(got) is np.float64 and got == slow_two_launch_sum(lay, prod)
        assert abs(got - math.fsum(prod)) <= 1e-13 * math.fsum(np.abs(prod))
        rows = tree.partials(prod)
        assert rows.shape == (g1 + g2,) and np.array_equal(rows[:g1], tree.launches[0].partials(prod)[:g1 or None] if g1 else rows[:0])
    a, b = rng.standard_normal(n), rng.standard_normal(n)
    assert tree.dot(a, b) == tree.sum(a * b)
    ints = rng.integers(-1000, 1000, n).astype(np.float64)
    assert tree.sum(ints) == ints.sum()
    if not g1:
        one = UnitTree.of(lay)
        assert np.array_equal(one.idx, tree.launches[0].idx) and one.sum(a) == tree.sum(a)


def test_two_launch_unit_tree_refuses_layouts_that_are_no_two_launches():
    rng = np.random.default_rng(8)
    lay = rank_unit_layout('full', 20, 6, 5, 2, rng)
    TwoLaunchUnitTree(lay)
    with pytest.raises(AssertionError, match='two launches'):
        TwoLaunchUnitTree(dict(lay, interior_slices=0))                # an interior launch ran, over no unit
    with pytest.raises(AssertionError, match='one launch'):
        TwoLaunchUnitTree(dict(lay, interior_grid=0))                  # one launch, yet both classes hold units
    twice = lay['slice_rows'].copy()
    twice[22] = twice[3]                                              # a boundary slice repeats an interior one's rows
    with pytest.raises(AssertionError, match='exactly once'):
        TwoLaunchUnitTree(dict(lay, slice_rows=twice))
    with pytest.raises(AssertionError):
        TwoLaunchUnitTree(dict(lay, window=True))
    # a launch over one class does not finish every row, and says so only when asked to
    units = [r[None, :] for r in lay['slice_rows']]
    part = UnitTree(units, 2, 4, first=20, count=6, whole=False)
    assert part.rows is None and int(part.idx[part.idx >= 0].min()) == 20 * 64
    with pytest.raises(AssertionError, match='exactly once'):
        UnitTree(units[:3] + units[4:], 2, 4)


@pytest.mark.parametrize('kind', ['full', 'tiles'])
def test_two_launch_unit_tree_discriminates(kind):
    """What the device's order could differ in without losing a row -- each changes bits of the sum of a generic vector (three
    vectors: at least one bit of any of the three sums): the boundary launch's partial rows laid BEFORE the interior launch's, one
    launch over all the units, the classes cut one unit too early or too late, and both launches' workgroups remapped with the
    summed grid instead of their own."""
    rng = np.random.default_rng(77)
    n_int, n_bnd, g1, g2 = 75, 22, 19, 6            # (neither grid a multiple of 8: the XCD order is no identity)
    lay = rank_unit_layout(kind, n_int, n_bnd, g1, g2, rng)
    tree = TwoLaunchUnitTree(lay)
    n = tree.rows[1]
    vecs = [rng.standard_normal(n) for _ in range(3)]
    ref = [tree.sum(v) for v in vecs]
    assert ref == [slow_two_launch_sum(lay, v) for v in vecs]
    bound = [2e-13 * math.fsum(np.abs(v)) for v in vecs]

    def differs(sums):
        assert all(abs(s - r) <= b for s, r, b in zip(sums, ref, bound))          # (still a valid summation of the same rows)
        return sums != ref
    # boundary partials first
    interior, boundary = tree.launches
    assert differs([np.float64(first_tree(np.concatenate([boundary.partials(v), interior.partials(v)]))) for v in vecs])
    # one launch over all the units, on a quarter of them as the start-up product runs
    one = UnitTree.of(dict(lay, grid=-(-(n_int + n_bnd) // 4)))
    assert differs([one.sum(v) for v in vecs])
    # ... and on g1 + g2 workgroups
    assert differs([UnitTree.of(dict(lay, grid=g1 + g2)).sum(v) for v in vecs])
    # the cut one unit off, either way
    key = 'interior_slices' if lay['sliced'] else 'interior_tiles'
    for off in (-1, 1):
        assert differs([TwoLaunchUnitTree(dict(lay, **{key: n_int + off})).sum(v) for v in vecs]), off
    # xcd_remap with the summed grid: wave v of workgroup b of either launch starts at unit xcd_remap(b, g1 + g2) * 4 + v of its class
    # (no permutation of the launch's own workgroups: rows are lost and taken twice -- the sum is no sum of these rows at all)
    us = slice_units(lay['slice_rows']) if lay['sliced'] else tile_units(lay['tiles'])

    def partials_remapped(first, count, grid, remap_grid, v_):
        ext = np.concatenate([v_, [0.0]])
        rows = []
        for b in range(grid):
            waves = []
            for v in range(4):
                acc = np.zeros(64)
                for u in range(xcd_remap(b, remap_grid) * 4 + v, count, grid * 4):
                    for step in us[first + u]:
                        acc = acc + ext[step]
                w = acc
                for off in (32, 16, 8, 4, 2, 1):
                    w = w + w[np.arange(64) ^ off]
                waves.append(w[0])
            rows.append(((waves[0] + waves[1]) + waves[2]) + waves[3])
        return np.array(rows)
    assert [first_tree(np.concatenate([partials_remapped(0, n_int, g1, g1, v), partials_remapped(n_int, n_bnd, g2, g2, v)])) for v in vecs] == ref
    assert [first_tree(np.concatenate([partials_remapped(0, n_int, g1, g1 + g2, v), partials_remapped(n_int, n_bnd, g2, g1 + g2, v)])) for v in vecs] != ref


def first_tree(partials):
    from device_order import _final_tree
    return _final_tree(np.asarray(partials, dtype=np.float64))
