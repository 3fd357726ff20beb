"""GPU (MI355X): the WHOLE free-running trajectory of every schedule on the two operator families that are no window operators
-- sliced rows (prcg_sell.hip: k_sell_win with window codes, k_sell_tiles with delta codes) and CSR-adaptive tiles
(prcg_kernels.hip: k_spmv_tiles) -- against the oracle (oracle/ne_oracle.py) run with the device's own summation order
(tests/device_order.py: UnitTree), as tests/test_trajectory_oracle.py holds the window operators.  Every inner product and
coefficient of every iteration bit for bit, x and r bit for bit: anything that depends on a session's history -- the prologue
sum of the one-launch pipelined iteration, partials pending across prcg_iterate calls, the three-launch Hestenes-Stiefel and
four-launch predict-and-recompute forms, the unfused Chronopoulos-Gear and Ghysels-Vanroose forms that only these operators
still run -- changes bits from the iteration at which it goes wrong.

Which launch sums which inner product on these operators (new_cg_variants_amd/csrc/prcg_session.cpp; "unit tree": the per-lane
sums of the slice / tile launch, block_reduce_store and the 256-thread final tree, UnitTree built from DeviceCSR.layout():
'slice_rows' or 'tiles', and the workgroups of the launch; "pair tree": the update kernels' two neighbouring elements per
thread, pair_sum; "pipelined update tree": k_pipe_update, device_dot):

  family              iterations                                                        start-up (prcg_solve_begin)
  pipe_*              iterate_pipe_fused: eng_fused -> launch_sell_pipe_fused /         launch_pipe_dots: all four by the
                      launch_pipe_fused, all four by the unit tree (summed by the next  pipelined update tree
                      launch's prologue, or by k_reduce_final)
  hs_cg, hs_pcg       iterate_hs_fused, the branch without window tiles: nu by          nu: launch_hs_init_dots, pair tree; mu:
                      launch_hs_update_xr (pair tree), launch_hs_update_p, mu by        dist_spmv kEpiDotXY, unit tree
                      eng_spmv kEpiDotXY (unit tree)
  pr_*, m_*           iterate_pr: nu by launch_pr_update (pair tree); mu, delta,        nu: launch_pr_init_dots, pair tree; mu,
                      gamma by overlapped_spmv -> eng_spmv kEpiPR (unit tree)           delta, gamma: dist_spmv kEpiPR, unit tree
  cg_cg, cg_pcg       iterate_cgcg: nu, eta by eng_spmv kEpiCG (unit tree), closed by   nu, eta: dist_spmv kEpiCG; mu: dist_spmv
                      k_reduce_final every iteration; mu derived                        kEpiDotXY: unit tree
  gv_cg, gv_pcg       iterate_gv: nu, eta by launch_gv_update1 (pair tree); the         nu, eta: launch_gv_update1; mu: launch_dot:
                      products have no epilogue; mu derived                             pair tree

Partial rows are always summed by the 256-thread tree, by the next launch's prologue (sum_prev_partials; k_spmv_tiles spells
the same tree out) or by k_reduce_final.  The workgroups of the launch come from the layout diagnostic, read once after
prcg_solve_begin and once after the run; the start-up products of Chronopoulos-Gear are two launches with two epilogues, so
every case asserts that the launch's workgroups follow from the table alone (a quarter of the units, or the per-CU knob).

Rows of the CSR-adaptive tiles longer than a tile are summed by a whole wave (64 lane sums and the butterfly), not left to
right: on such operators the oracle multiplies with LongRowOperator (tests/device_order.py), everywhere -- products, the
recorders' residual and A-norm -- and x and r are held to THAT oracle.

A case compares every iteration it runs and asserts that every inner product of the ORACLE is finite and nonzero at each.
After about k = 80 these well-conditioned operators are at rounding level: the recurrences stay deterministic, bit identity
still holds, and a stale partial shows most clearly there."""
import numpy as np
import pytest

from device_order import LongRowOperator, Routed, UnitTree, device_dot, first_mismatch, pair_sum, tile_cap_nnz
from oracle import ne_oracle as orc
from trajectory_common import CHUNKS, FIELD, FOUR, METHODS, holds_start, run_device, run_oracle

pytestmark = pytest.mark.gpu

ITERS = 100

# operator -> (matrix, knobs of the handle, what the handle must report).  Every handle: PRCG_SMALL=0.
#   family 'sliced' / 'csr'; codes 'window' / 'delta' (sliced rows); named: sorting windows, the slices name their rows
CUT = {'PRCG_SELL_WINDOW': '32', 'PRCG_SELL_MAX_OVERHEAD_PCT': '600'}
OPERATORS = {
    # fem_like_3d(16, 3), n = 12 288, rows of 24..81: 192 full slices; 900 tiles of at most 29 rows
    'fem16': ('fem16', {}, dict(family='sliced', codes='window', named=False)),
    'fem16_delta': ('fem16', {'PRCG_SELL_WINDOW': '0'}, dict(family='sliced', codes='delta', named=True)),        # (the planner sorts: sigma 256)
    'fem16_rowdelta': ('fem16', {'PRCG_SELL_WINDOW': '0', 'PRCG_SELL_SIGMA': '64'}, dict(family='sliced', codes='delta', named=False)),
    'fem16_csr': ('fem16', {'PRCG_SELL': '0'}, dict(family='csr')),
    # fem_irregular_3d(20), n = 24 025 = 375 * 64 + 25, rows of 14..100: padded window-code slices and a ragged last one;
    # delta codes under sorting windows; with 32 granules per slice 671 slices, most of them cut short
    'irr20': ('irr20', {}, dict(family='sliced', codes='window', named=False, ragged=True)),
    'irr20_named': ('irr20', {'PRCG_SELL_WINDOW': '0'}, dict(family='sliced', codes='delta', named=True, ragged=True)),
    'irr20_cut': ('irr20', CUT, dict(family='sliced', codes='window', named=False, cut=True)),
    # fem_like_3d(29, 3), n = 73 167: 1144 slices on one workgroup per CU, 5685 tiles on one workgroup per CU: >= 2 units per wave
    'fem29': ('fem29', {'PRCG_SELL_GRID_PER_CU': '1'}, dict(family='sliced', codes='window', named=False, per_wave=2)),
    'fem29_csr': ('fem29', {'PRCG_SELL': '0', 'PRCG_GRID_PER_CU': '1'}, dict(family='csr', per_wave=2)),
    # irregular_standin(20000): rows of 4..19 991, two of them longer than a tile (long rows); tiles of at most 34 rows
    's4_20k': ('s4_20k', {}, dict(family='csr', long_rows=True)),
    # irregular_standin(20000, mean_len=6): rows of 2..13 013 (two long rows), median 3 -- the smallest stand-in whose tiles hold
    # more than 64 rows: 266 tiles of up to 84 rows (two per lane), and with 1021-nonzero tiles 81 tiles of up to 256 rows
    # (the lane's third and fourth row: the loop behind process_tile's two prefetched batches)
    's4_short': ('s4_short', {}, dict(family='csr', long_rows=True, rows_per_lane=2)),
    's4_short4': ('s4_short', {'PRCG_TILE_STEPS': '4'}, dict(family='csr', long_rows=True, rows_per_lane=3)),
}
DEFER_OFF = {'PRCG_XP_DEFER': '0'}
ONE_PER_FAMILY = ['pipe_pr_pcg', 'pr_pcg', 'cg_cg', 'gv_cg', 'hs_pcg']
# (method, operator, knobs): every method on fem16's default plan and on its CSR-adaptive tiles, the pipelined Jacobi flavours
# also with PRCG_XP_DEFER=0 (the deferred store exists on window operators only: the knob must change nothing here); one method per
# routing family elsewhere, and pipe_p_m_pcg where the oracle allows it (the Meurant flavours break down on s4_20k: k = 39 to 85)
CASES = [(m, o, {}) for o in ('fem16', 'fem16_csr') for m in METHODS] + \
        [(m, o, DEFER_OFF) for o in ('fem16', 'fem16_csr') for m in METHODS if METHODS[m][1] == 'pipe' and METHODS[m][2]] + \
        [(m, o, {}) for o in ('fem16_delta', 'irr20', 'irr20_named', 'irr20_cut', 'fem29', 'fem29_csr', 's4_short')
         for m in ONE_PER_FAMILY + ['pipe_p_m_pcg']] + \
        [(m, o, {}) for o in ('fem16_rowdelta', 's4_20k', 's4_short4') for m in ONE_PER_FAMILY]


def case_id(c):
    return '-'.join([c[0], c[1]] + [f'{k[5:].lower()}{v}' for k, v in c[2].items()])


@pytest.fixture(scope='module')
def amd():
    from new_cg_variants_amd import _lib, device, problems
    return dict(L=_lib, device=device, problems=problems)


@pytest.fixture(scope='module')
def problem(amd):
    """matrix name -> (A, b, x_true, Jacobi of the oracle, inverse diagonal), built once per module and left unchanged"""
    P = amd['problems']
    make = {'fem16': lambda: P.fem_like_3d(16, 3), 'irr20': lambda: P.fem_irregular_3d(20), 'fem29': lambda: P.fem_like_3d(29, 3),
            's4_20k': lambda: P.irregular_standin(20000), 's4_short': lambda: P.irregular_standin(20000, mean_len=6)}
    cache = {}

    def get(name):
        if name not in cache:
            A = make[name]().tocsr()
            b, _, x_true = P.reference_rhs(A, A.shape[0])
            cache[name] = (A, b, x_true, orc.jacobi(A), 1 / A.diagonal())
        return cache[name]
    return get


@pytest.fixture(scope='module')
def trees():
    """(operator, workgroups) -> (layout, UnitTree): the tables of an operator are the same in every session, the model is built once"""
    cache = {}

    def get(operator, layout):
        key = (operator, layout['grid'], layout['waves_per_block'])
        if key not in cache:
            cache[key] = (layout, UnitTree.of(layout))
        assert same_tree(cache[key][0], layout), key
        return cache[key][1]
    return get


def oracle_dots(family, tree, start_tree):
    """(dot, dot0) for the oracle: which tree sums which inner product, in the order the oracle asks for them (module docstring;
    device_order.Routed: hs nu, mu; cg_cg and gv nu, eta (start: then mu); pr mu, delta, gamma, nu (start: nu first))"""
    if family == 'pipe':
        return Routed(tree.sum), device_dot
    if family == 'pr':
        return Routed(tree.sum, tree.sum, tree.sum, pair_sum), Routed(pair_sum, start_tree.sum, start_tree.sum, start_tree.sum)
    if family == 'cg':
        return Routed(tree.sum), Routed(start_tree.sum)
    if family == 'gv':
        return Routed(pair_sum), Routed(pair_sum)
    return Routed(pair_sum, tree.sum), Routed(pair_sum, start_tree.sum)         # hs: nu, mu


def same_tree(a, b):
    return a['grid'] == b['grid'] and a['waves_per_block'] == b['waves_per_block'] and np.array_equal(a['tiles'], b['tiles']) and \
        a['sliced'] == b['sliced'] and np.array_equal(a['slice_rows'], b['slice_rows'])


def check_plan(operator, knobs, want, A, s, lay):
    """the family, codes and table shape the case is there for, from the schedule flags and the tables read back from the device"""
    n = A.shape[0]
    assert not s['window'] and not lay['window'] and not s['small'] and not s['comm'] and not s['xp_deferred'], s
    assert s['sliced_rows'] == (want['family'] == 'sliced') and lay['sliced'] == s['sliced_rows'], s
    lens = np.diff(A.indptr)
    if want['family'] == 'sliced':
        assert s['window_codes'] == (want['codes'] == 'window') and s['sorted_windows'] == want['named'], s
        rows = lay['slice_rows']
        units = rows.shape[0]
        first = rows.max(axis=1) - (rows >= 0).sum(axis=1) + 1
        consecutive = np.array_equal(rows, np.where(rows >= 0, first[:, None] + np.arange(64)[None, :], -1))
        assert consecutive == (not want['named']), operator                   # named rows: some slice is no run of rows in lane order
        short = np.flatnonzero((rows < 0).any(axis=1))
        if want.get('ragged'):
            assert n % 64 and (rows >= 0).sum() == n and short.size >= 1
        if want.get('cut'):
            assert np.count_nonzero(short < units - 1) >= 100, short.size     # slices cut short in the middle of the table
    else:
        t = lay['tiles']
        units = t.shape[0]
        per_tile = t[:, 1] - t[:, 0]
        assert per_tile.sum() == n and per_tile.max() <= 256
        cap = tile_cap_nnz(s['tile_steps'])
        assert (lens.max() > cap) == bool(want.get('long_rows')), (lens.max(), cap)
        assert -(-per_tile.max() // 64) >= want.get('rows_per_lane', 1), per_tile.max()   # some lane finishes that many rows of one tile
    if lay['grid'] > 0:
        assert lay['waves_per_block'] == 4
        # the workgroups follow from the table, not from the launch's epilogue (its occupancy): every launch of the session has them
        assert lay['grid'] == -(-units // 4) or any(k.endswith('GRID_PER_CU') for k in knobs), (lay['grid'], units)
        assert units >= want.get('per_wave', 0) * lay['grid'] * 4, (units, lay['grid'])
    return units


@pytest.mark.parametrize('method,operator,knobs', CASES, ids=[case_id(c) for c in CASES])
def test_whole_trajectory_on_sliced_rows_and_csr_tiles(amd, problem, trees, method, operator, knobs):
    """`method` on a sliced-row or CSR-adaptive operator (module docstring: which launch sums what), PRCG_SMALL=0, 100
    iterations.  (a) all four recorders, so a reduction launch closes every iteration; (b) the recurrence residual only and
    prcg_iterate calls of 1, 2, 37 iterations and the rest: partials are summed by the next launch's prologue and stay pending
    across calls.  The oracle runs with the trees of the launches the layout diagnostics report.  Bit for bit in both modes:
    every inner product the method defines and the coefficients a, b of every iteration; the residual history of (a) and (b);
    in (b) x and r at k = 3, k = 40 and the end.  The recorder histories of (a): 1e-13 relative for the three 2-norms, 1e-11
    for the A-norm of the error (sums in another order by the recorder kernels), the bars of the window test."""
    whole_trajectory(amd, problem, trees, method, operator, knobs)


def whole_trajectory(amd, problem, trees, method, operator, knobs, x0=None, max_iter=ITERS):
    """the body of test_whole_trajectory_on_sliced_rows_and_csr_tiles.  x0: the start vector of every session and of the oracle
    (None: zeros); an array, or a callable (op, A, b) -> array that may run an earlier session on the handle
    (tests/warm_start_common.py).  With one, x and r right after prcg_solve_begin are held first: x == x0 and r == b - A x0 (A: the
    LongRowOperator where the operator has long rows), bit for bit."""
    L = amd['L']
    variant, family, jac, slots = METHODS[method]
    matrix, op_knobs, want = OPERATORS[operator]
    A, b, x_true, jacobi, inv_diag = problem(matrix)
    assert max_iter - 1 > sum(CHUNKS) + 1
    all_knobs = dict(op_knobs, PRCG_SMALL='0', **knobs)
    op = amd['device'].DeviceCSR(A, knobs=all_knobs)
    x0 = x0(op, A, b) if callable(x0) else x0
    runs = [run_device(L, op, getattr(L, variant), b, x_true, inv_diag if jac else None, max_iter, rec, x0=x0) for rec in (True, False)]
    op.close()
    for mode, r in zip('ab', runs):
        s = r['schedule']
        # no reduction launches in the one-launch pipelined and the three-launch Hestenes-Stiefel schedule; the others close
        # every iteration with k_reduce_final
        assert s['fused'] == (family in ('pipe', 'hs')), (mode, s)
        units = check_plan(operator, all_knobs, want, A, s, r['layout'])
        check_plan(operator, all_knobs, want, A, s, r['start_layout'])
        assert (r['layout']['grid'] > 0) == (family != 'gv'), r['layout']['grid']
        assert (r['start_layout']['grid'] > 0) == (family in ('pr', 'cg', 'hs')), r['start_layout']['grid']
    lay = runs[0]['layout']
    assert same_tree(runs[0]['start_layout'], runs[1]['start_layout'])
    keep = set(runs[1]['state'])
    assert keep == {1, 3, 40, max_iter - 1}
    A_dev = LongRowOperator(A, tile_cap_nnz(runs[0]['schedule']['tile_steps'])) if want.get('long_rows') else A
    if want.get('long_rows'):
        assert A_dev.long_rows.size >= 1
    if x0 is not None:
        for r in runs:
            holds_start(r['start'], 'xr', x0, b, A_dev)
    oracles = []
    for r in runs:
        if oracles and same_tree(r['layout'], runs[0]['layout']):
            oracles.append(oracles[0])
            continue
        tree = trees(operator, r['layout']) if r['layout']['grid'] > 0 else None
        start_tree = trees(operator, r['start_layout']) if r['start_layout']['grid'] > 0 else None
        dot, dot0 = oracle_dots(family, tree, start_tree)
        oracles.append(run_oracle(method, A_dev, b, x_true, jacobi, max_iter, dot, dot0, keep, x0=x0))
    cols = [FIELD[f] for _, f in slots]
    for mode, r, (rows, ref, snaps) in zip('ab', runs, oracles):
        want_dots = rows[:, cols]
        assert rows.shape[0] == max_iter and np.isfinite(want_dots).all() and (want_dots != 0).all(), \
            f'the oracle breaks down at k={int(np.argmin((np.isfinite(want_dots) & (want_dots != 0)).all(axis=1)))}: choose a shorter run'
        got = r['scalars'][:, [getattr(L, s) for s, _ in slots]]
        bad = first_mismatch(got, want_dots)
        assert bad < 0, f'({mode}) inner products {[f for _, f in slots]}: first mismatch at k={bad}: got {got[bad]} want {want_dots[bad]}'
        # a, b of iteration k: the step the oracle's state k-1 holds, the b its state k used
        want_coef = np.stack([rows[:-1, FIELD['alpha']], rows[1:, FIELD['beta']]], axis=1)
        bad = first_mismatch(r['coef'], want_coef)
        assert bad < 0, f'({mode}) coefficients: first mismatch at k={bad + 1}: got {r["coef"][bad]} want {want_coef[bad]}'
    assert np.array_equal(runs[0]['hist']['updated_residual_2_norm'], runs[1]['hist']['updated_residual_2_norm'])
    assert np.isfinite(runs[1]['hist']['updated_residual_2_norm']).all()
    snaps = oracles[1][2]
    for k in sorted(keep):
        for name, got, want_v in zip('xr', runs[1]['state'][k], snaps[k]):
            differ = int(np.count_nonzero(got != want_v))
            assert differ == 0, f'(b) {name} at k={k}: {differ} of {got.size} entries differ, worst {np.max(np.abs(got - want_v)):.3e}'
    ref = oracles[0][1]
    worst = {}
    for q in FOUR:
        assert np.isfinite(ref[q]).all() and np.isfinite(runs[0]['hist'][q]).all() and (ref[q] > 0).all(), q
        worst[q] = float(np.max(np.abs(runs[0]['hist'][q] - ref[q]) / ref[q]))
    print(f'{case_id((method, operator, knobs))}: {max_iter} iterations, {lay["grid"]} workgroups x {lay["waves_per_block"]} waves '
          f'({units} units): inner products, coefficients, x and r bit-exact; recorder histories worst rel. deviation ' +
          ', '.join(f'{q} {v:.1e}' for q, v in worst.items()))
    assert worst['updated_residual_2_norm'] <= 1e-13 and worst['residual_2_norm'] <= 1e-13 and worst['error_2_norm'] <= 1e-13, worst
    assert worst['error_A_norm'] <= 1e-11, worst
