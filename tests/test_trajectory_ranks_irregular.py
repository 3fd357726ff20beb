"""GPU (MI355X): the WHOLE free-running trajectory of sessions with 2-3 REAL ranks (threads of this process on one GPU,
tests/ranks_common.py) whose row blocks are NO window operators -- sliced rows (prcg_sell.hip) and CSR-adaptive tiles
(prcg_kernels.hip: k_spmv_tiles) -- against the oracle run with "every rank's own tree, then the ranks in rank order"
(tests/device_order.py: RankSum): tests/test_trajectory_ranks.py holds several ranks on window operators,
tests/test_trajectory_irregular.py these families on one GPU; the code that runs only with a communicator ON these families is
held here.  That is: overlapped_spmv's two launches (interior units into partial rows [0, g1), the units with a ghost column into
[g1, g1 + g2), one final tree), pipe_spmm_and_reduce's two launches over the ghost rows of the PAIR array -- fed by the all-reduce
path and by the gather path --, a rank without an interior slice (g1 == 0), the per-class encodings of the CSR-adaptive tiles, long
rows summed over owned and ghost columns, and slices whose stored column order steps back by more than one 16-bit delta code.

Which launch sums which inner product ON ONE RANK (prcg_session.cpp; every rank's value then goes through the rank-order sum;
"two-launch": TwoLaunchUnitTree built from the rank's DeviceCSR.layout(); "unit tree": UnitTree.of(the layout right after begin)):

  family        iterations                                                        start-up (prcg_solve_begin)
  pipe_*        iterate_pipe -> launch_pipe_update: all four by the pipelined     launch_pipe_dots: the same tree
                update tree over the rank's rows (device_sum); layout grid == 0
  hs            nu: launch_hs_update_xr (pair_sum); mu: overlapped_spmv           nu: pair_sum; mu: dist_spmv kEpiDotXY, ONE launch
                kEpiDotXY, two-launch                                             over all the rank's units (unit tree)
  pr / m        mu, delta, gamma: overlapped_spmv kEpiPR, two-launch; nu:         nu first: pair_sum; the other three: dist_spmv
                launch_pr_update (pair_sum)                                       kEpiPR, unit tree
  cg            nu, eta: overlapped_spmv kEpiCG, two-launch; mu derived           nu, eta, then mu: unit tree
  gv            nu, eta: launch_gv_update1 (pair_sum); mu derived                 pair_sum

Transports, pinned by knobs and asserted from schedule(): 'allreduce' (PRCG_GATHER=0: halo exchange, k_reduce_final, all-reduce) and,
for the pipelined methods, 'gather' (PRCG_GATHER_MAX_BYTES=32768: k_gather_pack, ONE all-gather, k_gather_unpack, which also puts
the ghost rows of the pair array into place).  Every rank reports comm and neither fused, fused_comm, peer nor window.

On operators with long rows (more nonzeros than a tile holds) the oracle multiplies with LongRowOperator(A_global, cap): a long
row is summed by its wave in STORED order, and a rank block stores a row's columns in the global order (ghost columns keep their
place, they are only renumbered), so the global matrix gives the order on every rank.

Cases: every one in the two modes of tests/ranks_trajectory_common.py.  ITERATIONS: 100 (fem23_delta: 60), or 10 fewer than the
first state at which the oracle's mu or nu, under THIS case's trees, is non-positive or not finite (BREAKS) -- the test computes
that state from its own oracle run of 100 iterations and asserts the table's figure against it, so a case cannot be shortened for
any other reason.  Jacobi nearly inverts the two stand-ins (s4_*): they run unpreconditioned methods only.

Not held this way: RCCL's own all-reduce order; the peer exchange (window operators only); stored-tilde and multi-RHS sessions on
several ranks; warm starts on these blocks."""
import numpy as np
import pytest

from device_order import LongRowOperator, RankSum, Routed, TwoLaunchUnitTree, UnitTree, device_sum, pair_sum, tile_cap_nnz
from oracle import ne_oracle as orc
from ranks_trajectory_common import hold_ranks_to_oracle, run_mode
from trajectory_common import ALL_METHODS

pytestmark = pytest.mark.gpu

FULL = 100               # iterations of the oracle run, and of a case whose oracle stays clear of a breakdown
# transport -> (handle knobs, schedule flags every rank must report)
NOT_WINDOW = dict(comm=True, fused=False, fused_comm=False, peer=False, window=False)
TRANSPORTS = {'allreduce': ({'PRCG_GATHER': '0'}, dict(NOT_WINDOW, gather=False)),
              'gather': ({'PRCG_GATHER_MAX_BYTES': '32768'}, dict(NOT_WINDOW, gather=True))}
THIN = [0, 2160, 3024, 5184]
# operator -> (matrix, ranks, row-block offsets or None: even, knobs of the handle, what the case is there for)
#   family 'sliced' / 'csr'; codes 'window' / 'delta' (sliced rows); empty_interior: the ranks without an interior unit
OPERATORS = {
    # fem_like_3d(12, 3), n = 5184: 34 interior + 7 boundary slices per rank, send list 432 rows
    'fem12': ('fem12', 2, None, {}, dict(family='sliced', codes='window')),
    'fem12_delta': ('fem12', 2, None, {'PRCG_SELL_WINDOW': '0'}, dict(family='sliced', codes='delta')),
    'fem12_csr': ('fem12', 2, None, {'PRCG_SELL': '0'}, dict(family='csr')),                      # 150 + 33 tiles per rank
    # the middle rank is 864 rows = two node planes, both next to a cut: no interior slice (g1 == 0), send list 864 rows
    'fem12_thin': ('fem12', 3, THIN, {}, dict(family='sliced', codes='window', empty_interior=(1,))),
    # fem_irregular_3d(12), n = 5277: ragged slices, cuts inside nodes
    'irr12': ('irr12', 3, None, {}, dict(family='sliced')),                  # (the planner picks the codes per rank)
    # irregular_standin(6000, ..): both tile classes on every rank; rows of 590 and 595 nonzeros on ranks 0 and 2 are long rows
    's4_6k': ('s4_6k', 3, None, {}, dict(family='csr', long_rows=(0, 2))),
    # irregular_standin(20000): EVERY tile reads ghost rows; rows 0 and 19999 (19 991 and 19 989 nonzeros) summed over owned and ghost columns
    's4_20k': ('s4_20k', 2, None, {}, dict(family='csr', long_rows=(0, 1), long_rows_read_ghosts=True, empty_interior=(0, 1))),
    # fem_like_3d(23, 3), n = 36 501: rank 1's rows start with ghost columns, numbered behind the owned ones -- a stored step back of
    # up to 19 910 columns, more than one 16-bit delta code spans (16 384): back-skip positions; fem_like_3d(22, 3) steps back 16 112
    'fem23_delta': ('fem23', 2, None, {'PRCG_SELL_WINDOW': '0'}, dict(family='sliced', codes='delta', back_skip=True, cap=60)),
}
ONE_PER_FAMILY = ['pipe_pr_pcg', 'pr_pcg', 'cg_cg', 'gv_cg', 'hs_pcg']
UNPRECONDITIONED = ['pipe_pr_cg', 'pr_cg', 'cg_cg', 'hs_cg']
DELTA_CODE_SPAN = 16384

# (method, operator) -> the oracle's first state with a non-positive or non-finite mu or nu under the case's trees (asserted)
# (fem12 reaches rounding level near k = 70: from there on the flavours that predict or derive an inner product meet such a state;
#  pipe_* and gv_* sum by the update kernels' trees over the rank's rows, so their figures follow the row blocks, not the family)
BREAKS = {('pipe_pr_pcg', 'fem12'): 86, ('pipe_p_pcg', 'fem12'): 81, ('pipe_pr_m_pcg', 'fem12'): 85, ('pipe_p_m_pcg', 'fem12'): 79,
          ('m_pcg', 'fem12'): 93, ('gv_cg', 'fem12'): 90, ('gv_pcg', 'fem12'): 75, ('pipe_p_cg', 'fem12'): 99, ('pipe_p_m_cg', 'fem12'): 97,
          ('pipe_pr_pcg', 'fem12_delta'): 86, ('gv_cg', 'fem12_delta'): 90, ('pipe_pr_pcg', 'fem12_csr'): 86, ('gv_cg', 'fem12_csr'): 90,
          ('pipe_pr_pcg', 'fem12_thin'): 86, ('gv_cg', 'fem12_thin'): 95}


def iterations(first_bad, cap=FULL):
    """`cap`, or 10 fewer than the oracle's first state with a non-positive or non-finite mu or nu if that is less"""
    return cap if first_bad < 0 else min(cap, first_bad - 10)


def case(method, operator, transport):
    it = iterations(BREAKS.get((method, operator), -1), OPERATORS[operator][4].get('cap', FULL))
    assert it >= 40, (method, operator, it)            # (a shorter case is replaced by its unpreconditioned sibling, not kept short)
    return (method, operator, transport, it)


# (method, operator, transport, iterations)
CASES = \
    [case(m, 'fem12', 'allreduce') for m in ALL_METHODS] + \
    [case(m, 'fem12', 'gather') for m in ALL_METHODS if ALL_METHODS[m][1] == 'pipe'] + \
    [case(m, o, 'allreduce') for o in ('fem12_delta', 'fem12_csr', 'fem12_thin', 'irr12') for m in ONE_PER_FAMILY] + \
    [case('pipe_pr_pcg', o, 'gather') for o in ('fem12_delta', 'fem12_csr', 'fem12_thin', 'irr12')] + \
    [case(m, o, 'allreduce') for o in ('s4_6k', 's4_20k') for m in UNPRECONDITIONED] + \
    [case(m, 'fem23_delta', 'allreduce') for m in ('pipe_pr_pcg', 'hs_pcg')]


def case_id(c):
    return '-'.join(str(f) for f in c)


@pytest.fixture(scope='module')
def amd():
    from new_cg_variants_amd import _lib, partition, problems
    return dict(L=_lib, problems=problems, partition=partition)


@pytest.fixture(scope='module')
def problem(amd):
    """matrix name -> (A, b, x_true, Jacobi of the oracle, inverse diagonal), built once per module and left unchanged"""
    P = amd['problems']
    make = {'fem12': lambda: P.fem_like_3d(12, 3), 'irr12': lambda: P.fem_irregular_3d(12), 'fem23': lambda: P.fem_like_3d(23, 3),
            's4_6k': lambda: P.irregular_standin(6000, mean_len=12, max_len=80, reach=900, seed=3), 's4_20k': lambda: P.irregular_standin(20000)}
    cache = {}

    def get(name):
        if name not in cache:
            A = make[name]().tocsr()
            b, _, x_true = P.reference_rhs(A, A.shape[0])
            cache[name] = (A, b, x_true, orc.jacobi(A), 1 / A.diagonal())
        return cache[name]
    return get


def units_of(lay):
    """(interior units, all units) of the family that runs"""
    return (lay['interior_slices'], lay['slice_rows'].shape[0]) if lay['sliced'] else (lay['interior_tiles'], lay['tiles'].shape[0])


def oracle_dots(family, offsets, ranks):
    """(dot, dot0) for the oracle: which tree sums which inner product on every rank, in the order the oracle asks for them
    (module docstring; device_order.Routed: hs nu, mu; cg nu, eta (start: then mu); pr mu, delta, gamma, nu (start: nu first))"""
    def every(make):
        return RankSum(offsets, [make(r) for r in ranks])
    if family == 'pipe':
        assert all(r['layout']['grid'] == 0 and r['start_layout']['grid'] == 0 for r in ranks), [r['layout']['grid'] for r in ranks]
        return Routed(every(lambda r: device_sum)), Routed(every(lambda r: device_sum))
    pair = every(lambda r: pair_sum)
    if family == 'gv':
        assert all(r['layout']['grid'] == 0 and r['start_layout']['grid'] == 0 for r in ranks)
        return Routed(pair), Routed(pair)
    assert all(r['start_layout']['grid'] > 0 and r['start_layout']['interior_grid'] == 0 for r in ranks), [r['start_layout']['grid'] for r in ranks]
    for r in ranks:
        n_int, n_all = units_of(r['layout'])
        assert r['layout']['grid'] > 0 and (r['layout']['interior_grid'] > 0) == (0 < n_int < n_all), (r['layout']['interior_grid'], n_int, n_all)
    two = every(lambda r: TwoLaunchUnitTree(r['layout']).sum)
    start = every(lambda r: UnitTree.of(r['start_layout']).sum)
    if family == 'pr':
        return Routed(two, two, two, pair), Routed(pair, start, start, start)
    if family == 'cg':
        return Routed(two), Routed(start)
    return Routed(pair, two), Routed(pair, start)                                    # hs: nu, mu


def same_tree(a, b):
    return all(a[k] == b[k] for k in ('grid', 'waves_per_block', 'interior_grid', 'interior_waves_per_block', 'interior_tiles', 'sliced',
                                      'interior_slices')) and np.array_equal(a['tiles'], b['tiles']) and np.array_equal(a['slice_rows'], b['slice_rows'])


def shape_line(ranks):
    out = []
    for r in ranks:
        lay = r['layout']
        n_int, n_all = units_of(lay)
        out.append(f"{lay['interior_grid']}+{lay['grid']} workgroups ({n_all - n_int} of {n_all} {'slices' if lay['sliced'] else 'tiles'} boundary, {n_int} interior)")
    return ', '.join(out)


def row_of_entry(A_local):
    return np.repeat(np.arange(A_local.shape[0]), np.diff(A_local.indptr))


def stored_step_back(A_local):
    """the largest step back between two columns a row stores one after the other (0: none)"""
    row = row_of_entry(A_local)
    d = A_local.indices[:-1].astype(np.int64) - A_local.indices[1:]
    return int(max(0, d[row[:-1] == row[1:]].max()))


def check_rank_plan(operator, want, A_local, n_local, s, lay, rank):
    """the family, codes and row classes the case is there for, from one rank's schedule flags and the tables read back from its
    device; the interior / boundary cut of the unit table against the rank's own block: a row is boundary iff it has a ghost column"""
    assert not s['small'] and not lay['window'], (operator, rank, s)
    assert s['sliced_rows'] == (want['family'] == 'sliced') and lay['sliced'] == s['sliced_rows'], (operator, rank, s)
    ghost_row = np.zeros(n_local, dtype=bool)
    ghost_row[row_of_entry(A_local)[A_local.indices >= n_local]] = True
    n_int, n_all = units_of(lay)
    if lay['sliced']:
        assert 'codes' not in want or s['window_codes'] == (want['codes'] == 'window'), (operator, rank, s)
        rows = lay['slice_rows']
        assert lay['interior_tiles'] >= 0 and 0 <= n_int <= n_all
        assert np.array_equal(np.sort(rows[rows >= 0]), np.arange(n_local)), (operator, rank)
        has_ghost = np.array([ghost_row[r[r >= 0]].any() for r in rows])
        assert not has_ghost[:n_int].any(), f'{operator} rank {rank}: an interior slice holds a row with a ghost column'
        assert has_ghost[n_int:].all(), f'{operator} rank {rank}: a slice behind the {n_int} interior ones holds no row with a ghost column'
    else:
        assert lay['interior_slices'] == 0 and lay['slice_rows'].shape[0] == 0
        t = lay['tiles']
        has_ghost = np.array([ghost_row[rb:re].any() for rb, re in t])
        assert not has_ghost[:n_int].any() and has_ghost[n_int:].all(), (operator, rank, n_int)
        assert (t[:, 1] - t[:, 0]).sum() == n_local
    assert (n_int == 0) == (rank in want.get('empty_interior', ())), f'{operator} rank {rank}: {n_int} interior units of {n_all}'
    assert n_int < n_all, (operator, rank)                    # every rank reads ghost rows
    assert lay['waves_per_block'] == 4


@pytest.mark.parametrize('method,operator,transport,iters', CASES, ids=[case_id(c) for c in CASES])
def test_whole_trajectory_of_a_multi_rank_session_on_sliced_rows_and_csr_tiles(amd, problem, method, operator, transport, iters):
    """Module docstring.  Bit for bit in both modes: every inner product the method defines and the coefficients a, b of every
    iteration on rank 0, and every rank's copy of them; one residual history; in (b) the concatenated x and r (with Jacobi r~,
    s~) at k = 1, 3, 40 and the end.  The recorder histories of (a): 1e-13 relative for the three 2-norms, 1e-11 for the A-norm
    of the error.  Every rank's unit table is cut into interior and boundary units where its own block says (a row with a ghost
    column is boundary), and the pattern the operator is there for holds: which ranks have no interior unit, which hold long rows,
    and for fem23_delta that rank 1 stores a step back beyond one delta code and rank 0 none."""
    L = amd['L']
    variant, family, jac, _ = ALL_METHODS[method]
    matrix, nranks, off, op_knobs, want = OPERATORS[operator]
    A, b, x_true, jacobi, inv_diag = problem(matrix)
    knobs, flags = TRANSPORTS[transport]
    knobs = dict(op_knobs, **knobs)
    long_rows = 'long_rows' in want

    def product(out):
        steps = [o['schedule']['tile_steps'] for o in out]
        assert len(set(steps)) == 1, steps
        return LongRowOperator(A, tile_cap_nnz(steps[0]))
    runs = [run_mode(L, A, method, nranks, knobs, False, off, inv_diag, iters, rec, product=product if long_rows else None) for rec in (True, False)]
    offsets = runs[0][0]
    assert np.array_equal(offsets, runs[1][0])
    _, parts = amd['partition'].split_serial(A, nranks, off)
    for mode, (_, ranks) in zip('ab', runs):
        for q, r in enumerate(ranks):
            assert all(r['schedule'][k] == v for k, v in flags.items()), (mode, q, flags, r['schedule'])
            for lay in (r['start_layout'], r['layout']):
                check_rank_plan(operator, want, parts[q][0].tocsr(), int(offsets[q + 1] - offsets[q]), r['schedule'], lay, q)
    A_dev = product(runs[0][1]) if long_rows else A
    if long_rows:
        owner = np.searchsorted(offsets, A_dev.long_rows, side='right') - 1
        assert sorted(set(owner.tolist())) == list(want['long_rows']), (A_dev.long_rows, owner)
        if want.get('long_rows_read_ghosts'):                      # the wave-wide sum runs over owned AND ghost columns
            for row, q in zip(A_dev.long_rows, owner):
                cols = A.indices[A.indptr[row]:A.indptr[row + 1]]
                mine = (cols >= offsets[q]) & (cols < offsets[q + 1])
                assert mine.any() and not mine.all(), row
    if want.get('back_skip'):
        back = [stored_step_back(p[0].tocsr()) for p in parts]
        assert back[0] == 0 and back[1] > DELTA_CODE_SPAN, back
    cap = want.get('cap', FULL)
    hold_ranks_to_oracle(L, case_id((method, operator, transport, iters)), method, A_dev, b, x_true, jacobi, runs,
                         oracle_dots(family, offsets, runs[0][1]), iters, FULL, lambda kb: iterations(kb, cap), same_tree, shape_line)
