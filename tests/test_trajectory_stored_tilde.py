"""GPU (MI355X): the WHOLE free-running trajectory of the STORED-TILDE schedule -- every session with a point-block Jacobi
preconditioner (uniform or variable blocks, set by the caller or built on the device) or a host-callback preconditioner --
against the oracle (oracle/ne_oracle.py) run with the same M^-1 as a callable and the device's own summation order
(tests/device_order.py), as tests/test_trajectory_oracle.py and tests/test_trajectory_irregular.py hold the other schedules.
In these sessions (prcg_session.cpp: Session::stored_tilde) fused, hs_fused, pr_fused and cg_fused are all off; r~, s~, w~, u~
are vectors in memory that apply_prec fills, and the update kernels take their `a.ut != nullptr` / `a.d == nullptr` branches.
Every inner product and coefficient of every iteration bit for bit, x and r -- and the stored u~, w~ of the pipelined
flavours -- bit for bit: a stale u~, a w~ of the wrong iteration or a wrong slot of partB changes bits from the iteration at
which it happens (tests/test_device_order.py shows that for the model's side on the CPU).

Which launch sums which inner product in a stored-tilde session, on EVERY operator family (new_cg_variants_amd/csrc/
prcg_session.cpp; "pipelined update tree": k_pipe_update, thread t elements t and t + 256 of a trip, device_dot; "pair tree":
k_hs_update_xr / k_pr_update / k_gv_update1 / k_dot, thread t elements 2t and 2t + 1, pair_sum -- k_dot read from the kernel:
i = (block * trips) * 512 + 2 * thread, then e = 0, 1, block_reduce_store, chunking(n) workgroups; "tile tree": the per-lane sums
of the product launch, its block reduction and the 256-thread final tree -- OneLaunchTree on window operators, UnitTree on sliced
rows and CSR-adaptive tiles, built from DeviceCSR.layout()):

  family              iterations                                                        start-up (prcg_solve_begin)
  pipe_*_pcg          iterate_pipe: launch_pipe_update with a.ut (u~, w~ loaded as      begin_pipe: r~, s~, u~ by apply_prec;
                      vectors), all four and rr by the pipelined update tree, closed    launch_pipe_dots: all four by the
                      by launch_reduce_final; then eng_spmm2 (no epilogue) and the      pipelined update tree
                      block-Jacobi pair launch or two callback calls (u~, w~)
  hs_pcg              iterate_hs: launch_hs_update_xr without M^-1 (its nu slot holds   launch_hs_init_dots (r.r), then nu:
                      r.r), apply_prec(r), nu by launch_dot(r~, r) (pair tree);         launch_dot, pair tree; mu: dist_spmv
                      launch_hs_update_p; mu by the product with kEpiDotXY (tile tree)  kEpiDotXY, tile tree
  pr_pcg, m_pcg       iterate_pr -> pr_spmv_and_reduce, stored-tilde branch: nu by      nu: launch_pr_init_dots, pair tree; mu,
                      launch_pr_update (pair tree); product kEpiNone; apply_prec(s);    delta, gamma: the same three launch_dot
                      mu, delta, gamma by three launch_dot into slots 0, 1, 2 of        (pr_spmv_and_reduce at k = 0), pair tree
                      partB (pair tree)
  cg_pcg              iterate_cgcg: launch_hs_update_xr (x, r), apply_prec(r), nu and   nu, eta: dist_spmv kEpiCG; mu: dist_spmv
                      eta by the product with kEpiCG (tile tree), closed by             kEpiDotXY: tile tree
                      launch_reduce_final every iteration; mu derived
  gv_pcg              iterate_gv: nu, eta by launch_gv_update1 (pair tree; w~ left to   nu, eta: launch_gv_update1; mu: launch_dot:
                      the caller), apply_prec(w); the products have no epilogue; mu     pair tree
                      derived

No product launch of the pipelined, predict-and-recompute and Ghysels-Vanroose sessions leaves partials: their layout
diagnostic reports no workgroups, at start-up and after the run, and their trees depend on n alone.  Hestenes-Stiefel and
Chronopoulos-Gear take the tile tree of the product launch the diagnostic reports, read once after prcg_solve_begin and once
after the run.  Every partial row is summed by launch_reduce_final (the 256-thread tree); nothing stays pending between
launches or prcg_iterate calls.

M^-1 of the oracle is the object the device runs: BlockJacobi / VarBlockJacobi called (their __call__ carries the kernel's
bits by contract, tests/test_block_jacobi.py, tests/test_block_jacobi_var.py); for blocks BUILT ON THE DEVICE a callable made
from the blocks read back, which are asserted equal to the invert_blocks restatement; the caller's own function for a host
callback (a tridiagonal solve: the staging copy, and the stride-2 sources w and u of the pair array).

A case compares every iteration it runs and asserts that every inner product of the ORACLE is finite and nonzero at each."""
import numpy as np
import pytest

from device_order import OneLaunchTree, Routed, UnitTree, chunking, device_sum, first_mismatch, pair_sum
from trajectory_common import CHUNKS, FIELD, FOUR, METHODS, holds_start, run_device, run_oracle

pytestmark = pytest.mark.gpu

# operator -> (matrix, knobs of the handle, family the handle must report).  Every handle: PRCG_SMALL=0.
OPERATORS = {
    'bcsstk03': ('bcsstk03', {}, 'window'),                  # golden, n = 112: one 128-row tile
    'nos7': ('nos7', {}, 'window'),                          # golden, n = 729: six 128-row tiles
    'lap2d_300': ('lap2d_300', {}, 'window'),                # laplace_2d(300, 200), n = 60 000: 938 tiles, workgroups no multiple of 8
    'fem16': ('fem16', {}, 'sliced'),                        # fem_like_3d(16, 3), n = 12 288: 192 full slices
    'fem16_csr': ('fem16', {'PRCG_SELL': '0'}, 'csr'),       # ... as 900 CSR-adaptive tiles
    'irr20': ('irr20', {}, 'sliced'),                        # fem_irregular_3d(20), n = 24 025 = 375 * 64 + 25: a ragged last slice
    'irr20_csr': ('irr20', {'PRCG_SELL': '0'}, 'csr'),
}
# preconditioner -> (kind, argument).  'bj': BlockJacobi(A, bs), inverses from the host; 'bjv': VarBlockJacobi(A, partition);
# 'bj_built' / 'bjv_built': the blocks built on the device (begin(..., block_jacobi=(bs, None)) / block_jacobi_var=(ptr, None));
# 'callback': the tridiagonal solve of test_gpu_parity.py::test_host_callback_preconditioner on the host
PRECS = {
    'bs3': ('bj', 3), 'bs4': ('bj', 4), 'bs7': ('bj', 7), 'bs8': ('bj', 8),
    'nodal': ('bjv', 'nodal'),                               # fem_irregular_blocks(20): blocks of 1, 3 and 6
    'cyc8': ('bjv', 'cyc8'),                                 # block sizes 1, 2, .. 8, 1, 2, .. (the last one cut to fit)
    'built3': ('bj_built', 3), 'built_nodal': ('bjv_built', 'nodal'),
    'tridiag': ('callback', None),
}
ALL = [m for m in METHODS if m.endswith('_pcg')]
ONE_PER_FAMILY = ['pipe_pr_pcg', 'pipe_p_m_pcg', 'pr_pcg', 'cg_pcg', 'gv_pcg', 'hs_pcg']
# (operator, preconditioner, methods, iterations).  112 = 37 * 3 + 1, 729 = 182 * 4 + 1, 60 000 = 8571 * 7 + 3: short last blocks.
# Lengths stay below the oracle's own breakdowns.  First iteration with a non-positive mu or nu of the oracle run 260 iterations
# under the trees of this schedule (the pipelined, predict-and-recompute and Ghysels-Vanroose families, whose trees depend on n
# alone; hs_pcg and cg_pcg, which take the product launch's tree, have none within their runs -- the case asserts it):
# bcsstk03 bs = 3 k = 231 (gv_pcg; pipe_p_m_pcg 237), bcsstk03 bs = 8 k = 98 (gv_pcg; pipe_p_m_pcg 99), nos7 bs = 4 k = 90
# (pipe_p_m_pcg), fem16 k = 90 (gv_pcg; pipe_p_pcg, pipe_p_m_pcg 93), irr20 k = 148 to 151 (pipe_p_m_pcg, gv_pcg), bcsstk03
# with blocks of 1..8 k = 213 (gv_pcg), nos7 under the tridiagonal solve k = 95 (pipe_p_m_pcg), lap2d_300 none
GROUPS = [
    ('bcsstk03', 'bs3', ALL, 200),
    ('nos7', 'bs4', ONE_PER_FAMILY, 80), ('bcsstk03', 'bs8', ONE_PER_FAMILY, 80), ('lap2d_300', 'bs7', ONE_PER_FAMILY, 150),
    ('fem16', 'bs3', ALL, 80), ('fem16_csr', 'bs3', ALL, 80),
    ('irr20', 'nodal', ONE_PER_FAMILY, 100), ('irr20_csr', 'built_nodal', ONE_PER_FAMILY, 100), ('irr20', 'built3', ONE_PER_FAMILY, 100),
    ('bcsstk03', 'cyc8', ONE_PER_FAMILY, 80),
    ('nos7', 'tridiag', ONE_PER_FAMILY, 80),
]
CASES = [(m, o, p, it) for o, p, ms, it in GROUPS for m in ms]
# family -> the state vectors read in mode (b): x and r, the stored u~ and w~ of the pipelined flavours, and every other vector
# both sides keep -- the other stored companions r~, s~ (w~ of Ghysels-Vanroose), the directions and the products
VECTORS = {'pipe': ('x', 'r', 'ut', 'wt', 'rt', 'st', 'p', 's', 'w', 'u'), 'hs': ('x', 'r', 'rt', 'p', 's'), 'pr': ('x', 'r', 'rt', 'st', 'p', 's'),
           'cg': ('x', 'r', 'rt', 'p', 's', 'w'), 'gv': ('x', 'r', 'rt', 'st', 'wt', 'p', 's', 'w', 'u')}


def case_id(c):
    return '-'.join([c[0], c[1], c[2], str(c[3])])


@pytest.fixture(scope='module')
def amd():
    import new_cg_variants_amd.cg_variants as cgv
    from new_cg_variants_amd import _lib, device, problems
    return dict(L=_lib, device=device, problems=problems, cgv=cgv)


@pytest.fixture(scope='module')
def problem(amd, matrices):
    """matrix name -> (A, b, x_true), built once per module and left unchanged"""
    P = amd['problems']
    make = {'lap2d_300': lambda: P.laplace_2d(300, 200), 'fem16': lambda: P.fem_like_3d(16, 3), 'irr20': lambda: P.fem_irregular_3d(20)}
    cache = {}

    def get(name):
        if name not in cache:
            if name in make:
                A = make[name]().tocsr()
                b, _, x_true = P.reference_rhs(A, A.shape[0])
            else:
                A, z = matrices[name]
                b, x_true = z['b'], z['x_true']
            cache[name] = (A, b, x_true)
        return cache[name]
    return get


def cyclic_partition(n):
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(len(sizes) % 8 + 1, n - sum(sizes)))
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


@pytest.fixture(scope='module')
def preconditioner(amd, problem):
    """(matrix, preconditioner name) -> the host object of that preconditioner, built once per module: BlockJacobi /
    VarBlockJacobi (LAPACK inverses, handed to the device), DeviceBlockJacobi / DeviceVarBlockJacobi (the invert_blocks
    restatement of the device build), or the tridiagonal solve"""
    cgv, cache = amd['cgv'], {}

    def partition(matrix, which):
        return amd['problems'].fem_irregular_blocks(20) if which == 'nodal' else cyclic_partition(problem(matrix)[0].shape[0])

    def get(matrix, name):
        if (matrix, name) not in cache:
            A = problem(matrix)[0]
            kind, arg = PRECS[name]
            if kind == 'bj':
                M = cgv.BlockJacobi(A, arg)
            elif kind == 'bjv':
                M = cgv.VarBlockJacobi(A, partition(matrix, arg))
            elif kind == 'bj_built':
                M = cgv.DeviceBlockJacobi(A, arg)
            elif kind == 'bjv_built':
                M = cgv.DeviceVarBlockJacobi(A, partition(matrix, arg))
            else:
                import scipy.sparse as sp
                import scipy.sparse.linalg as spla
                lu = spla.splu(sp.diags([A.diagonal(-1), A.diagonal(), A.diagonal(1)], [-1, 0, 1], format='csc'))   # SPD tridiagonal part

                def M(v):
                    return lu.solve(np.asarray(v, dtype=np.float64))
            cache[(matrix, name)] = M
        return cache[(matrix, name)]
    return get


@pytest.fixture(scope='module')
def trees():
    """(operator, workgroups, waves) -> (layout, tile tree): the tables of an operator are the same in every session"""
    cache = {}

    def get(operator, layout):
        key = (operator, layout['grid'], layout['waves_per_block'])
        if key not in cache:
            cache[key] = (layout, OneLaunchTree(layout) if layout['window'] else UnitTree.of(layout))
        assert same_tree(cache[key][0], layout), key
        return cache[key][1]
    return get


def same_tree(a, b):
    return a['grid'] == b['grid'] and a['waves_per_block'] == b['waves_per_block'] and np.array_equal(a['tiles'], b['tiles']) and \
        a['window'] == b['window'] and a['sliced'] == b['sliced'] and np.array_equal(a['slice_rows'], b['slice_rows'])


def oracle_dots(family, tree, start_tree):
    """(dot, dot0) for the oracle: which tree sums which inner product, in the order the oracle asks for them (module docstring;
    device_order.Routed: hs nu, mu; cg_cg and gv nu, eta (start: then mu); pr mu, delta, gamma, nu (start: nu first))"""
    if family == 'pipe':
        return Routed(device_sum), Routed(device_sum)
    if family in ('pr', 'gv'):
        return Routed(pair_sum), Routed(pair_sum)
    if family == 'cg':
        return Routed(tree.sum), Routed(start_tree.sum)
    return Routed(pair_sum, tree.sum), Routed(pair_sum, start_tree.sum)         # hs: nu, mu


def device_preconditioner(kind, arg, M):
    """the keyword of DeviceCSR.begin (run_device) for this preconditioner"""
    if kind == 'bj':
        return {'block_jacobi': (arg, M.inv_blocks)}
    if kind == 'bjv':
        return {'block_jacobi_var': (M.block_ptr, M.inv_blocks)}
    if kind == 'bj_built':
        return {'block_jacobi': (arg, None)}
    if kind == 'bjv_built':
        return {'block_jacobi_var': (M.block_ptr, None)}
    return {'preconditioner': M}


def check_plan(operator, family_wanted, A, s, lay):
    """the operator family and the table shape the case is there for, from the schedule flags and the tables read back"""
    n = A.shape[0]
    assert s['window'] == lay['window'] == (family_wanted == 'window'), s
    assert s['sliced_rows'] == lay['sliced'] == (family_wanted == 'sliced'), s
    if family_wanted == 'window':
        t = lay['tiles']
        assert t[0, 0] == 0 and t[-1, 1] == n and (t[1:, 0] == t[:-1, 1]).all()
        if operator in ('bcsstk03', 'nos7'):
            assert lay['rows_per_tile'] == 128 and t.shape[0] == -(-n // 128)      # one / six tiles, two rows per lane
        if operator == 'lap2d_300':
            assert t.shape[0] == 938
        return t.shape[0]
    if family_wanted == 'sliced':
        rows = lay['slice_rows']
        assert (rows >= 0).sum() == n
        if operator == 'irr20':
            assert n % 64 and (rows[-1] < 0).any()                                  # the ragged last slice
        return rows.shape[0]
    per_tile = lay['tiles'][:, 1] - lay['tiles'][:, 0]
    assert per_tile.sum() == n and per_tile.max() <= 256
    return per_tile.shape[0]


@pytest.mark.parametrize('method,operator,prec,max_iter', CASES, ids=[case_id(c) for c in CASES])
def test_whole_trajectory_of_the_stored_tilde_schedule(amd, problem, preconditioner, trees, method, operator, prec, max_iter):
    """`method` with a block-Jacobi or host-callback preconditioner (module docstring: which launch sums what), PRCG_SMALL=0.
    (a) all four recorders, one prcg_iterate call; (b) the recurrence residual only and prcg_iterate calls of 1, 2, 37
    iterations and the rest.  The oracle runs with the same M^-1 as a callable and the trees of the table.  Bit for bit in
    both modes: every inner product the method defines and the coefficients a, b of every iteration; the residual history
    of (a) and (b); in (b) x and r at k = 1, 3, 40 and the end, in the pipelined flavours the stored u~ and w~ there
    against the oracle's (w~: the recurrence in the 'p' flavours, M^-1 w in the 'pr' flavours), and with them every other
    state vector both sides keep (VECTORS: r~, s~, p, s, w, u as the family has them).  The recorder histories of
    (a): 1e-13 relative for the three 2-norms, 1e-11 for the A-norm of the error (sums in another order by the recorder
    kernels), the bars of the other two trajectory tests."""
    whole_trajectory(amd, problem, preconditioner, trees, method, operator, prec, max_iter)


def whole_trajectory(amd, problem, preconditioner, trees, method, operator, prec, max_iter, x0=None):
    """the body of test_whole_trajectory_of_the_stored_tilde_schedule.  x0: the start vector of every session and of the oracle
    (None: zeros); an array, or a callable (op, A, b) -> array that may run an earlier session on the handle
    (tests/warm_start_common.py).  With one, the state right after prcg_solve_begin is held first: x == x0 and r == b - A x0, bit
    for bit, and every vector of VECTORS equal to the oracle's state 0."""
    L = amd['L']
    variant, family, jac, slots = METHODS[method]
    assert jac
    matrix, op_knobs, family_wanted = OPERATORS[operator]
    A, b, x_true = problem(matrix)
    n = A.shape[0]
    kind, arg = PRECS[prec]
    M = preconditioner(matrix, prec)
    assert max_iter - 1 > sum(CHUNKS) + 1
    vectors = VECTORS[family]
    op = amd['device'].DeviceCSR(A, knobs=dict(op_knobs, PRCG_SMALL='0'))
    x0 = x0(op, A, b) if callable(x0) else x0
    runs = [run_device(L, op, getattr(L, variant), b, x_true, None, max_iter, rec, vectors=vectors, x0=x0, **device_preconditioner(kind, arg, M))
            for rec in (True, False)]
    blocks = op.get_block_jacobi() if kind == 'bj_built' else op.get_block_jacobi_var() if kind == 'bjv_built' else None
    op.close()
    if blocks is not None:
        # the blocks the device built are the restatement's, bit for bit; the oracle applies what was read back
        want_blocks = M.inv_blocks
        assert blocks.shape == want_blocks.shape and np.array_equal(blocks, want_blocks), int(np.count_nonzero(blocks != want_blocks))
        M = amd['cgv'].DeviceBlockJacobi(A, arg) if kind == 'bj_built' else amd['cgv'].DeviceVarBlockJacobi(A, M.block_ptr)
        if kind == 'bjv_built':
            M._layout()
        M._inv_blocks = np.ascontiguousarray(blocks)
    with_tile_tree = family in ('hs', 'cg')
    if x0 is not None:
        for r in runs:
            holds_start(r['start'], vectors, x0, b, A)
    for mode, r in zip('ab', runs):
        s = r['schedule']
        # the stored-tilde schedule: no one-launch or prologue-summed form of any family, not the one-workgroup solver
        assert not s['fused'] and not s['small'] and not s['comm'] and not s['xp_deferred'], (mode, s)
        assert s['block_jacobi'] == (kind != 'callback') and s['block_jacobi_var'] == kind.startswith('bjv'), (mode, s)
        for lay in (r['start_layout'], r['layout']):
            units = check_plan(operator, family_wanted, A, s, lay)
            assert (lay['grid'] > 0) == with_tile_tree, (mode, lay['grid'])
            if with_tile_tree and family_wanted != 'window':
                assert lay['waves_per_block'] == 4 and lay['grid'] == -(-units // 4), (lay['grid'], units)
        if with_tile_tree and operator == 'lap2d_300':
            assert r['layout']['grid'] % 8 != 0, r['layout']['grid']                # the remainder branch of xcd_remap
    lay = runs[0]['layout']
    assert same_tree(runs[0]['start_layout'], runs[1]['start_layout'])
    keep = set(runs[1]['state'])
    assert keep == {1, 3, 40, max_iter - 1}
    oracles = []
    for r in runs:
        if oracles and same_tree(r['layout'], runs[0]['layout']):
            oracles.append(oracles[0])
            continue
        tree = trees(operator, r['layout']) if with_tile_tree else None
        start_tree = trees(operator, r['start_layout']) if with_tile_tree else None
        dot, dot0 = oracle_dots(family, tree, start_tree)
        oracles.append(run_oracle(method, A, b, x_true, M, max_iter, dot, dot0, keep | ({0} if x0 is not None else set()), vectors=vectors, x0=x0))
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
    for r, (_, _, at) in zip(runs, oracles) if x0 is not None else ():
        for name, got, want_v in zip(vectors, r['start'], at[0]):
            assert np.array_equal(got, want_v), f'{name} right after prcg_solve_begin: {int(np.count_nonzero(got != want_v))} of {got.size} entries differ'
    for k in sorted(keep):
        for name, got, want_v in zip(vectors, runs[1]['state'][k], snaps[k]):
            differ = int(np.count_nonzero(got != want_v))
            assert differ == 0, f'(b) {name} at k={k}: {differ} of {got.size} entries differ, worst {np.max(np.abs(got - want_v)):.3e}'
    ref = oracles[0][1]
    worst = {}
    for q in FOUR:
        assert np.isfinite(ref[q]).all() and np.isfinite(runs[0]['hist'][q]).all() and (ref[q] > 0).all(), q
        worst[q] = float(np.max(np.abs(runs[0]['hist'][q] - ref[q]) / ref[q]))
    shape = f'{lay["grid"]} workgroups x {lay["waves_per_block"]} waves ({units} units) of the product launch and ' if with_tile_tree else ''
    print(f'{case_id((method, operator, prec, max_iter))}: {max_iter} iterations, {shape}{chunking(n)[0]} workgroups x 4 waves of the '
          f'update kernels: inner products, coefficients, {", ".join(vectors)} bit-exact; recorder histories worst rel. deviation ' +
          ', '.join(f'{q} {v:.1e}' for q, v in worst.items()))
    assert worst['updated_residual_2_norm'] <= 1e-13 and worst['residual_2_norm'] <= 1e-13 and worst['error_2_norm'] <= 1e-13, worst
    assert worst['error_A_norm'] <= 1e-11, worst
