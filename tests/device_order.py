"""TEST INFRASTRUCTURE: NumPy emulation of the device's inner-product reduction tree.

The fused update kernels (new_cg_variants_amd/csrc/prcg_kernels.hip: k_pipe_update,
block_reduce_store, k_reduce_final) sum a product array in a fixed order:

  thread (block b, lane t): elements (b*trips + j)*512 + t, then + 256 + t, for j = 0..trips-1
  wave   : xor butterfly 32,16,8,4,2,1          block : waves 0..3 in order
  final  : one block (256 threads): thread t sums partials t, t+256, ...; butterfly;
           4 waves in order   (k_reduce_final)

Plugging ``device_dot`` into the oracle (``dot=``) makes the oracle's free-running
trajectory comparable with the device's bit for bit.

``OneLaunchTree`` is the same for the ONE-LAUNCH iteration (prcg_win.hip: k_win_tiles<2,fused>, the schedule
bench.py times and every solve uses by default): its inner products are summed

  lane l of wave (block b, wave v): rows rb + j*64 + l (j = 0..M-1) of tiles  slot, slot + W, slot + 2W, ...
                                    with slot = xcd_remap(b) * WPB + v,  W = grid * WPB  (in that order)
  wave  : xor butterfly             block : waves 0..WPB-1 in order  ->  one partial per workgroup
  final : the 256-thread tree over the workgroups' partials (thread t: partials t, t+256, ...; butterfly;
          4 waves in order) -- by every workgroup of the NEXT launch in its prologue (sum_prev_partials) or
          by k_reduce_final when a prcg_iterate call ends: the same tree either way

built from DeviceCSR.layout() (prcg.h: prcg_debug_layout: tile rows, grid, waves per workgroup).

EVERY launch of k_win_tiles that leaves inner-product partials sums them this way, whatever its epilogue (one per-lane
acc[5] over the wave's tiles, win_block_reduce_store, the 256-thread final tree): the one-launch predict-and-recompute,
Chronopoulos-Gear and Ghysels-Vanroose iterations, their two-launch forms, the Hestenes-Stiefel product launch and the
products with a dot epilogue at a session's start.  Only the workgroup count and the waves per workgroup differ from launch
to launch; layout() reports those of the session's last such launch.

The update kernels other than k_pipe_update (k_hs_update_xr, k_pr_update, k_gv_update1, k_dot: prcg_kernels.hip) give each
thread two NEIGHBOURING elements per trip -- thread (block b, lane t): elements (b*trips + j)*512 + 2t, then + 1 -- and the
same wave / block / final tree: ``pair_sum``.

``UnitTree`` is the tile tree of the two families that are no window operators -- sliced rows (prcg_sell.hip) and CSR-adaptive
tiles (prcg_kernels.hip: k_spmv_tiles), always four waves per workgroup: a wave's units (slices: one row per lane; tiles:
ceil(rows / 64) rows per lane) come from DeviceCSR.layout()'s 'slice_rows' (prcg_debug_slice_rows) or 'tiles'.  A row of the
CSR-adaptive tiles that is longer than a tile is summed by its whole wave: ``LongRowOperator`` is the matrix with those rows
multiplied that way.

SEVERAL RANKS (tests/test_trajectory_ranks.py): every rank sums ITS rows with its own tree and the ranks' values are added in rank
order, v = s[0]; v += s[r] -- ``RankSum``.  A rank's tree is one of the above built from that rank's layout(), or ``PeerLaunchTree``
(the one-launch iteration over the direct peer exchange: one wave is the communication wave, the others' tiles shift by one slot, a
few boundary tiles go to the communication wave) or ``TwoLaunchTree`` (a product with a dot epilogue run as an interior and a
boundary launch whose partial rows lie end to end under one final tree).  On sliced rows and CSR-adaptive tiles
(tests/test_trajectory_ranks_irregular.py) that product is ``TwoLaunchUnitTree``: UnitTree over each class of the unit table.

``Routed`` lets a schedule whose inner products come from different launches (Hestenes-Stiefel: nu from the update
kernel, mu from the tile launch) plug into the oracle: the oracle calls ``dot`` in a fixed order per advance.
"""
import numpy as np

ELEMS_PER_TRIP = 512
MAX_GRID = 2048
FINAL_THREADS = 256


def chunking(n):
    total = (n + ELEMS_PER_TRIP - 1) // ELEMS_PER_TRIP
    grid = max(1, min(total, MAX_GRID))
    trips = (total + grid - 1) // grid
    grid = max(1, (total + trips - 1) // trips) if trips > 0 else 1
    return grid, max(trips, 1)


def _butterfly(v):
    """lane-0 value of the xor butterfly over the last axis (length 64)."""
    off = 32
    while off >= 1:
        v = v[..., :off] + v[..., off:2 * off]
        off //= 2
    return v[..., 0]


def device_sum(prod):
    prod = np.asarray(prod, dtype=np.float64)
    n = prod.shape[0]
    grid, trips = chunking(n)
    padded = np.zeros(grid * trips * ELEMS_PER_TRIP)
    padded[:n] = prod
    a = padded.reshape(grid, trips, 2, 256)
    acc = np.zeros((grid, 256))
    # elements past n are never added on the device; adding +0.0 here is the same value
    for j in range(trips):
        for e in range(2):
            acc = acc + a[:, j, e, :]
    waves = _butterfly(acc.reshape(grid, 4, 64))              # (grid, 4)
    partial = waves[:, 0]
    for w in range(1, 4):
        partial = partial + waves[:, w]
    # final kernel
    rounds = (grid + FINAL_THREADS - 1) // FINAL_THREADS
    pp = np.zeros(rounds * FINAL_THREADS)
    pp[:grid] = partial
    pp = pp.reshape(rounds, FINAL_THREADS)
    t = np.zeros(FINAL_THREADS)
    for j in range(rounds):
        t = t + pp[j]
    nw = FINAL_THREADS // 64
    wf = _butterfly(t.reshape(nw, 64))
    out = wf[0]
    for w in range(1, nw):
        out = out + wf[w]
    return float(out)


def pair_sum(prod):
    """k_hs_update_xr / k_pr_update / k_gv_update1 / k_dot: thread t of block b sums elements (b*trips + j)*512 + 2t and + 1,
    j = 0..trips-1, in that order; then as device_sum.  Returns np.float64."""
    prod = np.asarray(prod, dtype=np.float64)
    n = prod.shape[0]
    grid, trips = chunking(n)
    padded = np.zeros(grid * trips * ELEMS_PER_TRIP)
    padded[:n] = prod
    a = padded.reshape(grid, trips, 256, 2)
    acc = np.zeros((grid, 256))
    for j in range(trips):
        for e in range(2):
            acc = acc + a[:, j, :, e]
    waves = _butterfly(acc.reshape(grid, 4, 64))
    partial = waves[:, 0]
    for w in range(1, 4):
        partial = partial + waves[:, w]
    return _final_tree(partial)


def pair_dot(a, b):
    return pair_sum(np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64))


def device_dot(a, b):
    return device_sum(np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64))


def xcd_remap(b, nb):
    """prcg_device.hpp: xcd_remap -- workgroup b of nb -> position in the XCD-contiguous work order."""
    xcd, idx = b & 7, b >> 3
    q, r = nb >> 3, nb & 7
    base = xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q
    return base + idx


def _final_tree(partial):
    """the 256-thread tree over one partial per workgroup (k_reduce_final / sum_prev_partials)"""
    grid = partial.shape[0]
    rounds = (grid + FINAL_THREADS - 1) // FINAL_THREADS
    pp = np.zeros(rounds * FINAL_THREADS)
    pp[:grid] = partial
    pp = pp.reshape(rounds, FINAL_THREADS)
    t = np.zeros(FINAL_THREADS)
    for j in range(rounds):
        t = t + pp[j]
    wf = _butterfly(t.reshape(FINAL_THREADS // 64, 64))
    out = wf[0]
    for w in range(1, FINAL_THREADS // 64):
        out = out + wf[w]
    return np.float64(out)        # (not a Python float: the oracle's nu / mu must give inf / nan at a breakdown, not raise)


class Routed:
    """dot(a, b) for the oracle that sends its i-th call to sums[i % len(sums)] (each a callable on the array of products):
    the order in which a ``*_start`` / ``*_advance`` of oracle/ne_oracle.py asks for its inner products is fixed --
    hs: nu, mu;  cg_cg and gv: nu, eta (start: then mu);  pr: mu, delta, gamma, nu (start: nu first)."""

    def __init__(self, *sums):
        self.sums, self.calls = sums, 0

    def __call__(self, a, b):
        s = self.sums[self.calls % len(self.sums)]
        self.calls += 1
        return np.float64(s(np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64)))


def first_mismatch(got, want):
    """first row at which two (iterations, slots) arrays differ in any bit, -1 if none.  NaN never equals NaN here: a
    trajectory comparison holds only where both sides are numbers."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = ~(got == want)
    bad = bad.reshape(bad.shape[0], -1).any(axis=1)
    return int(np.argmax(bad)) if bad.any() else -1


class OneLaunchTree:
    """The summation order of the inner products a launch of k_win_tiles leaves (the one-launch pipelined iteration and every
    other epilogue with partials): built from layout()'s tile rows, workgroups and waves per workgroup of that launch."""

    def __init__(self, layout):
        assert layout['window'] and layout['grid'] > 0, layout
        tiles = np.asarray(layout['tiles'], dtype=np.int64)
        grid, wpb = int(layout['grid']), int(layout['waves_per_block'])
        M = int(layout['rows_per_tile']) // 64
        nt = tiles.shape[0]
        W = grid * wpb
        per_wave = (nt + W - 1) // W
        # idx[b, v, step, lane] = row summed by that lane at that step, -1: none
        idx = -np.ones((grid, wpb, per_wave * M, 64), dtype=np.int64)
        lane = np.arange(64)
        for b in range(grid):
            for v in range(wpb):
                for i, t in enumerate(range(xcd_remap(b, grid) * wpb + v, nt, W)):
                    rb, re = tiles[t]
                    for j in range(M):
                        rows = rb + j * 64 + lane
                        idx[b, v, i * M + j] = np.where(rows < re, rows, -1)
        self.idx = idx
        self.grid, self.wpb = grid, wpb
        covered = np.sort(idx[idx >= 0])
        assert np.array_equal(covered, np.arange(tiles[:, 0].min(), tiles[:, 1].max())), 'every row summed exactly once'

    def sum(self, prod):
        prod = np.asarray(prod, dtype=np.float64)
        ext = np.concatenate([prod, [0.0]])            # index -1 -> +0.0 (adding it changes nothing: acc starts at +0.0)
        acc = np.zeros(self.idx.shape[:2] + (64,))
        for step in range(self.idx.shape[2]):
            acc = acc + ext[self.idx[:, :, step, :]]
        waves = _butterfly(acc)                        # (grid, wpb)
        partial = waves[:, 0]
        for v in range(1, self.wpb):
            partial = partial + waves[:, v]
        return _final_tree(partial)

    def dot(self, a, b):
        return self.sum(np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64))


RELAY_TILES = 8          # prcg_win.hip: kRelayTiles -- boundary tiles the communication wave of the peer exchange takes itself


class _TileWaves:
    """One launch of k_win_tiles with any assignment of tiles to waves: ``assign(b, v)`` -> the tiles (indices into `tiles`) wave
    v of workgroup b takes, in order.  lane l adds rows rb + j*64 + l (j = 0..M-1) of each, from +0.0; butterfly; waves 0..wpb-1
    in order -> ``partials(prod)``: one value per workgroup, in workgroup order (the rows of the launch's partials buffer)."""

    def __init__(self, tiles, M, grid, wpb, assign):
        grid, wpb = int(grid), int(wpb)
        assert grid > 0 and wpb > 0, (grid, wpb)
        mine = [[list(assign(b, v)) for v in range(wpb)] for b in range(grid)]
        steps = max(1, max(len(m) for row in mine for m in row)) * M
        # idx[b, v, step, lane] = row summed by that lane at that step, -1: none
        idx = -np.ones((grid, wpb, steps, 64), dtype=np.int64)
        lane = np.arange(64)
        for b in range(grid):
            for v in range(wpb):
                for i, t in enumerate(mine[b][v]):
                    rb, re = tiles[t]
                    for j in range(M):
                        rows = rb + j * 64 + lane
                        idx[b, v, i * M + j] = np.where(rows < re, rows, -1)
        self.idx, self.grid, self.wpb = idx, grid, wpb

    def partials(self, prod):
        ext = np.concatenate([np.asarray(prod, dtype=np.float64), [0.0]])     # index -1 -> +0.0 (acc starts at +0.0)
        acc = np.zeros(self.idx.shape[:2] + (64,))
        for step in range(self.idx.shape[2]):
            acc = acc + ext[self.idx[:, :, step, :]]
        waves = _butterfly(acc)                        # (grid, wpb)
        partial = waves[:, 0]
        for v in range(1, self.wpb):
            partial = partial + waves[:, v]
        return partial


def _assert_every_row_once(tiles, *launches):
    covered = np.sort(np.concatenate([l.idx[l.idx >= 0] for l in launches]))
    assert np.array_equal(covered, np.arange(tiles[:, 0].min(), tiles[:, 1].max())), 'every row summed exactly once'


class PeerLaunchTree:
    """OneLaunchTree's sibling for the one-launch iteration over the DIRECT PEER EXCHANGE (prcg_win.hip: k_win_tiles<.., DEF> with
    fz.px set): wave slot s = xcd_remap(b) * WPB + v; slot 0 is the launch's communication wave; every other wave takes tiles
    s - 1, s - 1 + (W - 1), ... below tend with W = grid * WPB.  A rank with 1..RELAY_TILES boundary tiles (the tiles behind
    layout()['interior_tiles']): tend = the interior tiles, and the communication wave takes the boundary tiles one after
    another; else tend = all tiles and the communication wave adds nothing.  Workgroup partials under the 256-thread tree
    (sum_prev_partials<5, WPB> of workgroup 0 of the next launch, or k_peer_collect): ``sum`` is ONE RANK's slot."""

    def __init__(self, layout):
        assert layout['window'] and layout['grid'] > 0, layout
        tiles = np.asarray(layout['tiles'], dtype=np.int64)
        grid, wpb = int(layout['grid']), int(layout['waves_per_block'])
        nt, nt_int = tiles.shape[0], int(layout['interior_tiles'])
        assert 0 <= nt_int <= nt, (nt_int, nt)
        W = grid * wpb
        self.relayed = 0 < nt - nt_int <= RELAY_TILES
        tend = nt_int if self.relayed else nt

        def assign(b, v):
            s = xcd_remap(b, grid) * wpb + v
            if s == 0:
                return range(nt_int, nt) if self.relayed else range(0)
            return range(s - 1, tend, W - 1)             # (W == 1: the launch is its communication wave alone -- no other slot)
        self.launch = _TileWaves(tiles, int(layout['rows_per_tile']) // 64, grid, wpb, assign)
        self.idx, self.grid, self.wpb = self.launch.idx, grid, wpb
        _assert_every_row_once(tiles, self.launch)

    def sum(self, prod):
        return _final_tree(self.launch.partials(prod))

    def dot(self, a, b):
        return self.sum(np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64))


class TwoLaunchTree:
    """A product with a dot epilogue as the two-kernel schedules run it WITH A COMMUNICATOR (prcg_session.cpp: overlapped_spmv):
    the interior tiles [0, interior_tiles) in one launch ('interior_grid' workgroups of 'interior_waves_per_block' waves, partial
    rows [0, g1)), the tiles that read ghost rows in a second ('grid' x 'waves_per_block', rows [g1, g1 + g2)), each with the plain
    assignment over ITS tiles (wave slot s takes its s-th, (s + W)-th, ... tile); ONE 256-thread tree over the g1 + g2 rows."""

    def __init__(self, layout):
        assert layout['window'] and layout['grid'] > 0 and layout['interior_grid'] > 0, {k: v for k, v in layout.items() if np.ndim(v) == 0}
        tiles = np.asarray(layout['tiles'], dtype=np.int64)
        nt, nt_int = tiles.shape[0], int(layout['interior_tiles'])
        assert 0 < nt_int < nt, (nt_int, nt)
        M = int(layout['rows_per_tile']) // 64

        def plain(first, count, grid, wpb):
            return _TileWaves(tiles, M, grid, wpb, lambda b, v: range(first + xcd_remap(b, grid) * wpb + v, first + count, grid * wpb))
        self.interior = plain(0, nt_int, int(layout['interior_grid']), int(layout['interior_waves_per_block']))
        self.boundary = plain(nt_int, nt - nt_int, int(layout['grid']), int(layout['waves_per_block']))
        _assert_every_row_once(tiles, self.interior, self.boundary)

    def sum(self, prod):
        return _final_tree(np.concatenate([self.interior.partials(prod), self.boundary.partials(prod)]))

    def dot(self, a, b):
        return self.sum(np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64))


class RankSum:
    """An inner product of a multi-rank session: rank r sums ITS rows [offsets[r], offsets[r + 1]) of the product array with its
    own tree (per_rank_sums[r], a callable on the rank's block in the rank's local row numbers -- ranks may carry different
    trees), and the ranks' sums are added in rank order STARTING FROM RANK 0's VALUE, v = s[0]; v += s[r] (k_gather_unpack,
    peer_collect, the all-reduce of tests/transport/threads_ccl.hip) -- not from 0.0: 0.0 + (-0.0) is +0.0."""

    def __init__(self, offsets, per_rank_sums):
        self.offsets = [int(o) for o in offsets]
        self.sums = list(per_rank_sums)
        assert len(self.offsets) == len(self.sums) + 1 and self.offsets[0] == 0 and all(a < b for a, b in zip(self.offsets, self.offsets[1:]))

    def slots(self, prod):
        prod = np.asarray(prod, dtype=np.float64)
        assert prod.shape == (self.offsets[-1],), (prod.shape, self.offsets[-1])
        return [np.float64(s(prod[lo:hi])) for s, lo, hi in zip(self.sums, self.offsets, self.offsets[1:])]

    def __call__(self, prod):
        s = self.slots(prod)
        v = s[0]
        for r in range(1, len(s)):
            v = v + s[r]
        return np.float64(v)

    def dot(self, a, b):
        return self(np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64))


def tile_units(tiles):
    """the units of CSR-adaptive tiles (process_tile) from layout()['tiles']: lane l of the tile's wave finishes rows rb + l,
    rb + 64 + l, ... below re -- ceil(rows / 64) steps; a long-row tile is one row, finished by lane 0 after the wave has summed it"""
    lane = np.arange(64)
    units = []
    for rb, re in np.asarray(tiles, dtype=np.int64):
        rows = rb + 64 * np.arange(-(-(re - rb) // 64))[:, None] + lane[None, :]
        units.append(np.where(rows < re, rows, -1))
    return units


def slice_units(slice_rows):
    """the units of sliced rows (slice_row) from layout()['slice_rows']: lane l finishes ONE row per slice -- rb + l, or the row
    the slice names for that lane; -1: an idle lane (a ragged, cut or padded slice)"""
    return [r[None, :] for r in np.asarray(slice_rows, dtype=np.int64)]


def _assert_rows_once(*launches):
    """the launches together finish every row of one contiguous range exactly once; returns the range"""
    covered = np.sort(np.concatenate([l.idx[l.idx >= 0] for l in launches]))
    assert covered.size > 0 and np.array_equal(covered, np.arange(covered[0], covered[-1] + 1)), 'every row summed exactly once'
    return int(covered[0]), int(covered[-1]) + 1


class UnitTree:
    """The summation order of the inner products a launch of the sliced-row kernels (prcg_sell.hip: k_sell_win, k_sell_tiles)
    or of the CSR-adaptive tile kernel (prcg_kernels.hip: k_spmv_tiles) leaves, whatever its epilogue:

      wave v of workgroup b takes UNITS (slices / tiles) xcd_remap(b, grid) * wpb + v, + grid * wpb, ... of the launch's table,
      in that order; one lane-private accumulator per inner product, starting at +0.0, adds the rows the lane finishes
      unit   : an ordered list of 64-lane row vectors, one per step, -1: the lane finishes no row in that step
      wave   : xor butterfly       block : waves 0..wpb-1 in order (block_reduce_store) -> ``partials``: one row per workgroup
      final  : the 256-thread tree -> ``sum``

    ``units``: a sequence of integer arrays of shape (steps, 64) -- steps may differ from unit to unit and may be 0.  A launch
    over ONE CLASS of the table (an overlapped product's interior or boundary launch) is handed the table from its first unit on:
    units [first, first + count), numbered from 0 within the launch.  Such a launch finishes only some of the rows (whole=False):
    that every row is finished exactly once is then asserted by whoever combines the launches (TwoLaunchUnitTree)."""

    def __init__(self, units, grid, wpb=4, first=0, count=None, whole=True):
        grid, wpb = int(grid), int(wpb)
        assert grid > 0 and wpb > 0, (grid, wpb)
        units = [np.asarray(u, dtype=np.int64).reshape(-1, 64) for u in units]
        first = int(first)
        count = len(units) - first if count is None else int(count)
        assert 0 <= first and 0 <= count and first + count <= len(units), (first, count, len(units))
        units = units[first:first + count]
        W = grid * wpb
        waves = []
        for b in range(grid):
            for v in range(wpb):
                mine = [units[t] for t in range(xcd_remap(b, grid) * wpb + v, len(units), W)]
                waves.append(np.concatenate(mine, axis=0) if mine else np.zeros((0, 64), dtype=np.int64))
        steps = max(w.shape[0] for w in waves)
        # idx[b, v, step, lane] = row summed by that lane at that step, -1: none
        idx = -np.ones((grid * wpb, steps, 64), dtype=np.int64)
        for i, w in enumerate(waves):
            idx[i, :w.shape[0]] = w
        self.idx = idx.reshape(grid, wpb, steps, 64)
        self.grid, self.wpb = grid, wpb
        self.rows = _assert_rows_once(self) if whole else None

    @classmethod
    def from_tiles(cls, layout):
        """CSR-adaptive tiles (tile_units), one launch over the whole table"""
        assert not layout['window'] and not layout['sliced'] and layout['grid'] > 0, {k: v for k, v in layout.items() if np.ndim(v) == 0}
        return cls(tile_units(layout['tiles']), layout['grid'], layout['waves_per_block'])

    @classmethod
    def from_slices(cls, layout):
        """sliced rows (slice_units), one launch over the whole table"""
        assert layout['sliced'] and layout['grid'] > 0, {k: v for k, v in layout.items() if np.ndim(v) == 0}
        return cls(slice_units(layout['slice_rows']), layout['grid'], layout['waves_per_block'])

    @classmethod
    def of(cls, layout):
        return cls.from_slices(layout) if layout['sliced'] else cls.from_tiles(layout)

    def partials(self, prod):
        """one value per workgroup, in workgroup order: the rows of the launch's partials buffer, before the final tree"""
        prod = np.asarray(prod, dtype=np.float64)
        ext = np.concatenate([prod, [0.0]])            # index -1 -> +0.0 (adding it changes nothing: acc starts at +0.0)
        acc = np.zeros(self.idx.shape[:2] + (64,))
        for step in range(self.idx.shape[2]):
            acc = acc + ext[self.idx[:, :, step, :]]
        waves = _butterfly(acc)                        # (grid, wpb)
        partial = waves[:, 0]
        for v in range(1, self.wpb):
            partial = partial + waves[:, v]
        return partial

    def sum(self, prod):
        return _final_tree(self.partials(prod))

    def dot(self, a, b):
        return self.sum(np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64))


class TwoLaunchUnitTree:
    """TwoLaunchTree's sibling on sliced rows and CSR-adaptive tiles: a product with a dot epilogue as the two-kernel schedules
    run it WITH A COMMUNICATOR (prcg_session.cpp: overlapped_spmv -> eng_spmv(which = 1), then (which = 2)).  The interior units
    -- slices [0, 'interior_slices') of 'slice_rows' on sliced rows, tiles [0, 'interior_tiles') on CSR-adaptive tiles -- run on
    'interior_grid' workgroups and leave partial rows [0, g1); the units with a ghost column, the rest of the table, run on 'grid'
    workgroups and leave rows [g1, g1 + g2).  Each launch is handed ITS class's table: wave v of workgroup b takes units
    xcd_remap(b, that launch's grid) * 4 + v, + 4 * that grid, ... counted from the class's first unit.  ONE 256-thread tree sums
    the g1 + g2 rows, interior first.  A rank with one class empty ('interior_grid' == 0: no interior slice, or no unit that reads
    a ghost row) launches the other class alone, on 'grid' workgroups: then this is UnitTree over that class."""

    def __init__(self, layout):
        assert not layout['window'] and layout['grid'] > 0, {k: v for k, v in layout.items() if np.ndim(v) == 0}
        units = slice_units(layout['slice_rows']) if layout['sliced'] else tile_units(layout['tiles'])
        n_int = int(layout['interior_slices'] if layout['sliced'] else layout['interior_tiles'])
        g1, g2, wpb = int(layout['interior_grid']), int(layout['grid']), int(layout['waves_per_block'])
        assert 0 <= n_int <= len(units) and len(units) > 0, (n_int, len(units))
        if g1 == 0:
            assert n_int in (0, len(units)), f'one launch, but {n_int} interior units of {len(units)}'
            self.launches = [UnitTree(units, g2, wpb, whole=False)]
        else:
            assert 0 < n_int < len(units), f'two launches, but {n_int} interior units of {len(units)}'
            self.launches = [UnitTree(units, g1, wpb, first=0, count=n_int, whole=False),
                             UnitTree(units, g2, wpb, first=n_int, count=len(units) - n_int, whole=False)]
        self.interior_units, self.units = n_int, len(units)
        self.rows = _assert_rows_once(*self.launches)

    def partials(self, prod):
        """the g1 + g2 partial rows as they lie in the buffer: the interior launch's, then the boundary launch's"""
        return np.concatenate([l.partials(prod) for l in self.launches])

    def sum(self, prod):
        return _final_tree(self.partials(prod))

    def dot(self, a, b):
        return self.sum(np.asarray(a, dtype=np.float64) * np.asarray(b, dtype=np.float64))


def long_row_sum(prod):
    """a long row of the CSR-adaptive tiles (process_tile: more nonzeros than the tile cap): lane l adds the products l, l + 64,
    ... left to right from +0.0, the wave butterfly gives the row result -- NOT SciPy's left-to-right sum."""
    prod = np.asarray(prod, dtype=np.float64)
    padded = np.zeros(-(-prod.shape[0] // 64) * 64)
    padded[:prod.shape[0]] = prod                      # (a lane past the end adds nothing; +0.0 here is the same value)
    acc = np.zeros(64)
    for chunk in padded.reshape(-1, 64):
        acc = acc + chunk
    return np.float64(_butterfly(acc))


def tile_cap_nnz(tile_steps):
    """most nonzeros of a CSR-adaptive tile (prcg_kernels.hip: kCap) for schedule()['tile_steps']; a longer row is a long row"""
    return 256 * int(tile_steps) - 3


class LongRowOperator:
    """A as the CSR-adaptive tile kernels multiply it: ``@`` is SciPy's product (every row left to right) except in rows
    with more than `cap` nonzeros, which are summed as the device sums them (long_row_sum).  Forwards what the oracle and
    the tests ask of an operator besides ``A @ v``: .shape and .diagonal()."""

    def __init__(self, A, cap):
        self.A, self.cap = A.tocsr(), int(cap)
        self.shape = self.A.shape
        self.long_rows = np.flatnonzero(np.diff(self.A.indptr) > self.cap)

    def diagonal(self):
        return self.A.diagonal()

    def __matmul__(self, v):
        y = self.A @ v
        v = np.asarray(v, dtype=np.float64)
        assert v.ndim == 1
        for i in self.long_rows:
            lo, hi = self.A.indptr[i], self.A.indptr[i + 1]
            y[i] = long_row_sum(self.A.data[lo:hi] * v[self.A.indices[lo:hi]])
        return y
