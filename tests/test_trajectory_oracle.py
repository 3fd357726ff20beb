"""GPU (MI355X): the WHOLE free-running trajectory of every default schedule on window operators against the oracle
(oracle/ne_oracle.py) run with the device's own summation order (tests/device_order.py) -- the second of the two
comparisons DESIGN.md section 2 names as well-posed on ill-conditioned matrices.  Every inner product and coefficient of
every iteration bit for bit, x and r bit for bit, hundreds of iterations: a stale partial row, a double-buffer swap gone
wrong, a race or a deferred store applied in the wrong phase changes bits from the iteration at which it happens
(tests/test_device_order.py shows that for the model's side on the CPU).

Which launch sums which inner product (new_cg_variants_amd/csrc/prcg_session.cpp; "tile tree": k_win_tiles' per-lane sums,
win_block_reduce_store and the 256-thread final tree, OneLaunchTree built from prcg_debug_layout's workgroups and waves per
workgroup of the launch; "pair tree": the update kernels' two neighbouring elements per thread, pair_sum; "pipelined update
tree": k_pipe_update, device_dot):

  family                  iterations                                                   start-up (prcg_solve_begin)
  pipe_*_pcg              iterate_pipe_fused: launch_win_pipe_fused, all four by the   launch_pipe_dots: all four by the
                          tile tree                                                    pipelined update tree
  pr_pcg, m_pcg           iterate_pr_fused: launch_win_pr_one (kEpiPROne / PROneJ /    nu: launch_pr_init_dots, pair tree; mu, delta,
                          PROneQ), all four by the tile tree                           gamma: dist_spmv with kEpiPR, tile tree
  cg_cg, cg_pcg, gv_cg    iterate_cg_one: launch_win_cg_one, nu and eta by the tile    cg: nu, eta dist_spmv kEpiCG and mu dist_spmv
  in one launch           tree (mu derived by the next launch / cg_flush)              kEpiDotXY, tile tree; gv: nu, eta
  gv_pcg, PRCG_CG_ONE=0   iterate_gv_fused / iterate_cgcg_fused: launch_win_gv_w /     launch_gv_update1 and mu launch_dot, pair tree
  in two launches         launch_win_cg_w, nu and eta by the tile tree
  hs_cg, hs_pcg           iterate_hs_fused: nu by launch_hs_update_xr (pair tree),     nu: launch_hs_init_dots, pair tree; mu:
                          mu by launch_win_hs (tile tree)                              dist_spmv kEpiDotXY, tile tree

Partial rows are always summed by the 256-thread tree: in the next launch's prologue (sum_prev_partials), or by
k_reduce_final when a recorder or the end of a prcg_iterate call closes the iteration.  The start-up tile launches run with
their own workgroup shape (another epilogue: the 128-row geometry of the golden matrices takes 4 waves there and 2 in the
packed predict-and-recompute and the Jacobi Chronopoulos-Gear launches): the test reads prcg_debug_layout once after
prcg_solve_begin and once after the run.

A case compares only iterations at which every inner product of the ORACLE is finite and nonzero, and asserts that this is
every iteration it runs."""
import numpy as np
import pytest

from device_order import OneLaunchTree, Routed, device_dot, first_mismatch, pair_sum
from oracle import ne_oracle as orc
from trajectory_common import CHUNKS, FIELD, FOUR, METHODS, holds_start, run_device, run_oracle

pytestmark = pytest.mark.gpu

# operator -> knobs of the handle (every handle: PRCG_SMALL=0, the one-workgroup solver of tiny systems has its own order)
OPERATORS = {
    'bcsstk03': {}, 'nos7': {},                              # golden, n = 112 / 729: one / six 128-row tiles, two rows per lane
    's3_small': {}, 's3_plain': {'PRCG_VALDICT': '0'},       # n = 20 000 band: 313 tiles, with and without value dictionary
    'lap2d_300': {},                                         # n = 60 000: 938 pattern tiles, a workgroup count that is no multiple of 8
    'lap3d_40': {},                                          # n = 64 000: 1000 pattern tiles
    'lap2d_400': {'PRCG_WIN_GRID_PER_CU': '1'},              # n = 160 000: 2500 tiles on at most one workgroup per CU: >= 2 tiles per wave
}
DEFER_OFF, PACK, UNPACK, TWO = {'PRCG_XP_DEFER': '0'}, {'PRCG_PR_PACK': '1'}, {'PRCG_PR_PACK': '0'}, {'PRCG_CG_ONE': '0'}
# the pipelined launch of a SHORT launch takes big workgroups (16 waves: 157 x 16 waves for the 2500 tiles of lap2d_400, one tile
# per wave -- that shape is held on s3_small, lap2d_300 and lap3d_40); with the four-wave workgroups of long launches the 2500
# tiles go to 256 x 4 waves, two or three each
SMALL_WG = {'PRCG_WIN_BIG': '0'}

# (method, operator, iterations, knobs).  Per method: a golden matrix (400 iterations with Jacobi, 800 without), an operator with
# hundreds of workgroups and the several-tiles-per-wave operator (150 iterations); lengths stay below the oracle's breakdowns
# (s3_small: hs_pcg and cg_pcg at k = 48, the Meurant pipelined flavours at k = 13: those take other operators; with the tile
# tree pipe_pr_m_pcg breaks down at k = 340 and pipe_p_m_pcg at k = 298 on bcsstk03 -- one tile: the same tree whatever the
# workgroup shape -- and at k = 118 to 129 on nos7 depending on it: bcsstk03 with 300 and 260 iterations).  Packed predict-and-recompute on bcsstk03, not
# nos7: with six 128-row tiles the packed launch (2 waves per workgroup) and the unpacked one a recorder forces (4 waves) are
# different trees, and the case asserts one residual history for both modes.
CASES = [
    ('pipe_pr_pcg', 'bcsstk03', 400, {}), ('pipe_pr_pcg', 'bcsstk03', 400, DEFER_OFF), ('pipe_pr_pcg', 's3_small', 150, {}),
    ('pipe_pr_pcg', 's3_plain', 150, DEFER_OFF), ('pipe_pr_pcg', 'lap2d_400', 150, SMALL_WG),
    ('pipe_p_pcg', 'nos7', 400, {}), ('pipe_p_pcg', 'nos7', 400, DEFER_OFF), ('pipe_p_pcg', 'lap2d_300', 150, {}),
    ('pipe_p_pcg', 'lap2d_300', 150, DEFER_OFF), ('pipe_p_pcg', 'lap2d_400', 150, SMALL_WG),
    ('pipe_pr_m_pcg', 'bcsstk03', 300, {}), ('pipe_pr_m_pcg', 'bcsstk03', 300, DEFER_OFF), ('pipe_pr_m_pcg', 'lap3d_40', 150, {}),
    ('pipe_pr_m_pcg', 'lap3d_40', 150, DEFER_OFF), ('pipe_pr_m_pcg', 'lap2d_400', 150, SMALL_WG),
    ('pipe_p_m_pcg', 'bcsstk03', 260, {}), ('pipe_p_m_pcg', 'bcsstk03', 260, DEFER_OFF),
    ('pipe_p_m_pcg', 'lap2d_300', 150, {}), ('pipe_p_m_pcg', 'lap2d_300', 150, DEFER_OFF), ('pipe_p_m_pcg', 'lap2d_400', 150, SMALL_WG),
    ('pr_pcg', 'nos7', 400, {}), ('pr_pcg', 's3_small', 150, {}), ('pr_pcg', 'lap2d_400', 150, {}),
    ('m_pcg', 'bcsstk03', 400, {}), ('m_pcg', 'lap3d_40', 150, {}), ('m_pcg', 'lap2d_400', 150, {}),
    ('pr_cg', 'bcsstk03', 800, PACK), ('pr_cg', 'nos7', 800, UNPACK), ('pr_cg', 's3_plain', 150, PACK), ('pr_cg', 'lap2d_300', 150, UNPACK),
    ('pr_cg', 'lap2d_400', 150, PACK), ('pr_cg', 'lap2d_400', 150, UNPACK),
    ('m_cg', 'bcsstk03', 800, PACK), ('m_cg', 'nos7', 800, UNPACK), ('m_cg', 'lap3d_40', 150, PACK), ('m_cg', 's3_small', 150, UNPACK),
    ('m_cg', 'lap2d_400', 150, PACK), ('m_cg', 'lap2d_400', 150, UNPACK),
    ('cg_cg', 'nos7', 800, {}), ('cg_cg', 's3_plain', 150, {}), ('cg_cg', 'lap2d_400', 150, {}),
    ('cg_cg', 'bcsstk03', 800, TWO), ('cg_cg', 'lap2d_300', 150, TWO), ('cg_cg', 'lap2d_400', 150, TWO),
    ('cg_pcg', 'bcsstk03', 400, {}), ('cg_pcg', 'lap3d_40', 150, {}), ('cg_pcg', 'lap2d_400', 150, {}),
    ('gv_cg', 'nos7', 800, {}), ('gv_cg', 's3_small', 150, {}), ('gv_cg', 'lap2d_400', 150, {}),
    ('gv_pcg', 'nos7', 400, {}), ('gv_pcg', 'lap2d_300', 150, {}), ('gv_pcg', 'lap2d_400', 150, {}),
    ('hs_cg', 'bcsstk03', 800, {}), ('hs_cg', 's3_plain', 150, {}), ('hs_cg', 'lap3d_40', 150, {}), ('hs_cg', 'lap2d_400', 150, {}),
    ('hs_pcg', 'nos7', 400, {}), ('hs_pcg', 'lap2d_300', 150, {}), ('hs_pcg', 'lap2d_400', 150, {}),
]


def case_id(c):
    return '-'.join([c[0], c[1], str(c[2])] + [f'{k[5:].lower()}{v}' for k, v in c[3].items()])


@pytest.fixture(scope='module')
def amd():
    from new_cg_variants_amd import _lib, device, problems
    return dict(L=_lib, device=device, problems=problems)


@pytest.fixture(scope='module')
def problem(amd, matrices):
    """operator name -> (A, b, x_true, Jacobi of the oracle, inverse diagonal), built once per module and left unchanged"""
    P = amd['problems']
    make = {'s3_small': lambda: P.WORKLOADS['s3_small']['make'](), 's3_plain': lambda: P.WORKLOADS['s3_small']['make'](),
            'lap2d_300': lambda: P.laplace_2d(300, 200), 'lap3d_40': lambda: P.laplace_3d(40, 40, 40),
            'lap2d_400': lambda: P.laplace_2d(400, 400)}
    cache = {}

    def get(name):
        if name not in cache:
            if name in make:
                A = make[name]()
                b, _, x_true = P.reference_rhs(A, A.shape[0])
            else:
                A, z = matrices[name]
                b, x_true = z['b'], z['x_true']
            cache[name] = (A, b, x_true, orc.jacobi(A), 1 / A.diagonal())
        return cache[name]
    return get


def oracle_dots(family, tree, start_tree):
    """(dot, dot0) for the oracle: which tree sums which inner product, in the order the oracle asks for them (module docstring)"""
    if family == 'pipe':
        return Routed(tree.sum), device_dot
    if family == 'pr':
        return Routed(tree.sum), Routed(pair_sum, start_tree.sum, start_tree.sum, start_tree.sum)
    if family == 'cg':
        return Routed(tree.sum), Routed(start_tree.sum)
    if family == 'gv':
        return Routed(tree.sum), Routed(pair_sum)
    return Routed(pair_sum, tree.sum), Routed(pair_sum, start_tree.sum)         # hs: nu, mu


def same_tree(a, b):
    return a['grid'] == b['grid'] and a['waves_per_block'] == b['waves_per_block'] and np.array_equal(a['tiles'], b['tiles'])


@pytest.mark.parametrize('method,operator,max_iter,knobs', CASES, ids=[case_id(c) for c in CASES])
def test_whole_trajectory_of_the_default_schedule(amd, problem, method, operator, max_iter, knobs):
    """The default schedule of `method` on a window operator (module docstring: which launch sums what), PRCG_SMALL=0.
    (a) all four recorders, so a reduction launch closes every iteration (and a packed predict-and-recompute state is
    unpacked: kEpiPROne instead of kEpiPROneQ); (b) the recurrence residual only and prcg_iterate calls of 1, 2, 37 iterations
    and the rest: partials are summed by the next launch's prologue and stay pending across calls, the deferred (x,p) store
    of the pipelined launch alternates by parity.  The oracle runs with the trees of the launches the layout diagnostic
    reports.  Bit for bit in both modes: every inner product the method defines and the coefficients a, b of every
    iteration; the residual history of (a) and (b); in (b) x and r at k = 3, k = 40 and the end (multiply, then
    add, no FMA).  The recorder histories of (a): 1e-13 relative for the three 2-norms, 1e-11 for the A-norm of the error
    (sums in another order by the recorder kernels)."""
    whole_trajectory(amd, problem, method, operator, max_iter, knobs)


def whole_trajectory(amd, problem, method, operator, max_iter, knobs, x0=None):
    """the body of test_whole_trajectory_of_the_default_schedule.  x0: the start vector of every session and of the oracle (None:
    zeros); an array, or a callable (op, A, b) -> array that may run an earlier session on the handle (tests/warm_start_common.py).
    With one, x and r right after prcg_solve_begin are held first: x == x0 and r == b - A x0, bit for bit."""
    L = amd['L']
    variant, family, jac, slots = METHODS[method]
    A, b, x_true, jacobi, inv_diag = problem(operator)
    assert max_iter - 1 > sum(CHUNKS)
    op = amd['device'].DeviceCSR(A, knobs=dict(OPERATORS[operator], PRCG_SMALL='0', **knobs))
    x0 = x0(op, A, b) if callable(x0) else x0
    runs = [run_device(L, op, getattr(L, variant), b, x_true, inv_diag if jac else None, max_iter, rec, x0=x0) for rec in (True, False)]
    op.close()
    if x0 is not None:
        for r in runs:
            holds_start(r['start'], 'xr', x0, b, A)
    for mode, r in zip('ab', runs):
        s = r['schedule']
        # the schedule of the table: window tiles, no reduction launches (one launch per iteration; hs and the two-launch forms:
        # two), not the one-workgroup solver; which of the one- / two-launch and packed / unpacked forms runs follows from the
        # knobs alone (prcg_solve_begin: cg_one, pr_packed)
        assert s['window'] and s['fused'] and not s['small'] and not s['comm'], (mode, s)
        if family == 'pipe':
            assert s['xp_deferred'] == (mode == 'b' and knobs.get('PRCG_XP_DEFER') != '0'), (mode, s)
        assert r['layout']['window'] and r['layout']['grid'] > 0, r['layout']
        assert (r['start_layout']['grid'] > 0) == (family in ('pr', 'cg', 'hs')), r['start_layout']
    lay = runs[0]['layout']
    W = lay['grid'] * lay['waves_per_block']
    if operator == 'lap2d_400':
        assert lay['tiles'].shape[0] >= 2 * W and lay['grid'] <= 256, (lay['grid'], lay['waves_per_block'])     # every wave sums two or more tiles
    if operator == 'lap2d_300':
        assert lay['grid'] % 8 != 0, lay['grid']                      # the remainder branch of xcd_remap
    if operator in ('bcsstk03', 'nos7'):
        assert lay['rows_per_tile'] == 128                            # two rows per lane
    assert same_tree(runs[0]['start_layout'], runs[1]['start_layout'])
    keep = set(runs[1]['state'])
    assert keep == {1, 3, 40, max_iter - 1}
    oracles = []
    for r in runs:
        if oracles and same_tree(r['layout'], runs[0]['layout']):
            oracles.append(oracles[0])
            continue
        tree = OneLaunchTree(r['layout'])
        start_tree = OneLaunchTree(r['start_layout']) if r['start_layout']['grid'] > 0 else None
        dot, dot0 = oracle_dots(family, tree, start_tree)
        oracles.append(run_oracle(method, A, b, x_true, jacobi, max_iter, dot, dot0, keep, x0=x0))
    cols = [FIELD[f] for _, f in slots]
    for mode, r, (rows, ref, snaps) in zip('ab', runs, oracles):
        want = rows[:, cols]
        assert rows.shape[0] == max_iter and np.isfinite(want).all() and (want != 0).all(), \
            f'the oracle breaks down at k={int(np.argmin((np.isfinite(want) & (want != 0)).all(axis=1)))}: choose a shorter run'
        got = r['scalars'][:, [getattr(L, s) for s, _ in slots]]
        bad = first_mismatch(got, want)
        assert bad < 0, f'({mode}) inner products {[f for _, f in slots]}: first mismatch at k={bad}: got {got[bad]} want {want[bad]}'
        # a, b of iteration k: the step the oracle's state k-1 holds, the b its state k used
        want_coef = np.stack([rows[:-1, FIELD['alpha']], rows[1:, FIELD['beta']]], axis=1)
        bad = first_mismatch(r['coef'], want_coef)
        assert bad < 0, f'({mode}) coefficients: first mismatch at k={bad + 1}: got {r["coef"][bad]} want {want_coef[bad]}'
    assert np.array_equal(runs[0]['hist']['updated_residual_2_norm'], runs[1]['hist']['updated_residual_2_norm'])
    assert np.isfinite(runs[1]['hist']['updated_residual_2_norm']).all()
    snaps = oracles[1][2]
    for k in sorted(keep):
        for name, got, want in zip('xr', runs[1]['state'][k], snaps[k]):
            differ = int(np.count_nonzero(got != want))
            assert differ == 0, f'(b) {name} at k={k}: {differ} of {got.size} entries differ, worst {np.max(np.abs(got - want)):.3e}'
    ref = oracles[0][1]
    worst = {}
    for q in FOUR:
        assert np.isfinite(ref[q]).all() and np.isfinite(runs[0]['hist'][q]).all() and (ref[q] > 0).all(), q
        worst[q] = float(np.max(np.abs(runs[0]['hist'][q] - ref[q]) / ref[q]))
    print(f'{case_id((method, operator, max_iter, knobs))}: {max_iter} iterations, {lay["grid"]} workgroups x {lay["waves_per_block"]} waves '
          f'({lay["tiles"].shape[0]} tiles): inner products, coefficients, x and r bit-exact; recorder histories worst rel. deviation ' +
          ', '.join(f'{q} {v:.1e}' for q, v in worst.items()))
    assert worst['updated_residual_2_norm'] <= 1e-13 and worst['residual_2_norm'] <= 1e-13 and worst['error_2_norm'] <= 1e-13, worst
    assert worst['error_A_norm'] <= 1e-11, worst
