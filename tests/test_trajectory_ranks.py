"""GPU (MI355X): the WHOLE free-running trajectory of sessions with 2-4 REAL ranks (threads of this process on one GPU,
tests/ranks_common.py) against the oracle (oracle/ne_oracle.py) run with "every rank's own tree, then the ranks in rank order" as
its summation order (tests/device_order.py: RankSum) -- what tests/test_trajectory_oracle.py holds the single-GPU schedules to.
The arithmetic of a multi-rank run is deterministic: the distributed product is the global one bit for bit (asserted by
run_ranks), Jacobi and the updates are elementwise, each rank sums its own rows in a fixed tree and the ranks' sums are added
v = s[0]; v += s[r] (k_gather_unpack; peer_collect; ncclAllReduce of tests/transport/threads_ccl.hip).  A boundary tile that
reads ghost rows of the wrong parity of the exchange buffer, a halo one iteration stale, a slot added twice or out of order
on one rank, a boundary tile's partial lost when the communication wave takes it: each changes bits from the iteration at which
it happens (tests/test_device_order.py shows that for the model's side on the CPU).

Which launch sums which inner product ON ONE RANK (new_cg_variants_amd/csrc/prcg_session.cpp, prcg_win.hip; every rank's value
then goes through the rank-order sum; "pipelined update tree": k_pipe_update, device_sum; "pair tree": k_hs_update_xr /
k_pr_update / k_gv_update1, pair_sum; the trees below are built from each rank's own DeviceCSR.layout()):

  schedule (flags)                       iterations                                                  start-up (prcg_solve_begin)
  pipe_*, two-kernel with a              iterate_pipe -> launch_pipe_update: all four by the          launch_pipe_dots -> launch_reduce_final
  communicator (comm, not fused_comm)    pipelined update tree over the rank's rows; closed by        -> all-reduce: pipelined update tree
                                         launch_reduce_final + all-reduce, or (gather) by
                                         k_gather_pack's 256-thread tree + k_gather_unpack
  pipe_*, one launch with the gather     iterate_pipe_fused_comm: k_win_tiles<.., DEF> over ALL the   the same
  (fused_comm, gather)                   rank's tiles at the deferred form's grid, plain assignment
                                         (OneLaunchTree); k_gather_pack's tree; k_gather_unpack
  pipe_*, one launch over the peer       the same launch with fz.px: wave slot 0 is the               the same (rank 0's slot of "iteration
  exchange (fused_comm, peer)            communication wave, the others take tiles s - 1, s - 1 +     0" carries the reduced values, the
                                         (W - 1), ..; <= 8 boundary tiles go to the communication     others 0.0)
                                         wave (PeerLaunchTree); sum_prev_partials<5, WPB> of the
                                         next launch's workgroup 0 or k_peer_collect (flush_pending:
                                         end of a prcg_iterate call, before a recorder); peer_collect
  hs_cg / hs_pcg, two-kernel             iterate_hs: nu by launch_hs_update_xr (pair tree); mu by     nu: launch_hs_init_dots, pair tree; mu:
                                         overlapped_spmv kEpiDotXY: interior launch into partial      dist_spmv kEpiDotXY, ONE launch over all
                                         rows [0, g1), boundary launch into [g1, g1 + g2), one        the rank's tiles (OneLaunchTree)
                                         final tree over g1 + g2 rows (TwoLaunchTree)
  pr_cg / pr_pcg, two-kernel             iterate_pr: nu by launch_pr_update (pair tree); mu, delta,   nu: launch_pr_init_dots, pair tree; the
                                         gamma by overlapped_spmv kEpiPR (TwoLaunchTree)              other three: dist_spmv kEpiPR, one launch
  cg_cg / cg_pcg, two-kernel             iterate_cgcg: nu, eta by overlapped_spmv kEpiCG              nu, eta: dist_spmv kEpiCG; mu: dist_spmv
                                         (TwoLaunchTree); mu derived                                  kEpiDotXY: one launch each
  gv_cg / gv_pcg, two-kernel             iterate_gv: nu, eta by launch_gv_update1 (pair tree); the    nu, eta: launch_gv_update1; mu: launch_dot:
                                         product has no epilogue; mu derived                          pair tree

A recorder's product (record(): dist_spmv, one launch) leaves the layout report as the iteration left it.  The two launches of
an overlapped product are reported as 'grid' / 'waves_per_block' (boundary) and 'interior_grid' / 'interior_waves_per_block'.

Cases (every one in two modes, as tests/trajectory_common.py: (a) all four recorders, one prcg_iterate call; (b) the recurrence
residual only, prcg_iterate calls of 1, 2, 37 iterations and the rest, state vectors read after each).  ITERATIONS: 200, or 10
fewer than the first state at which the oracle's mu or nu, under THIS case's trees, is non-positive or not finite (BREAKS) -- the
test computes that state from its own oracle run of 200 iterations and asserts the table's figure against it, so a case cannot be
shortened for any other reason.  Three methods meet such a state within the first 10 on s3_small with Jacobi (see BREAKS), which
would leave no run at all: they run every iteration before it (5 and 6).

Not held this way: RCCL's own all-reduce between processes (the library does not fix the order in which it adds the ranks'
values; the stand-in transport of these tests adds them in rank order, as the engine's own kernels do)."""
import numpy as np
import pytest

from device_order import OneLaunchTree, PeerLaunchTree, RankSum, Routed, TwoLaunchTree, device_sum, pair_sum
from oracle import ne_oracle as orc
from ranks_trajectory_common import chunk_lengths, first_breakdown, hold_ranks_to_oracle, run_mode, state_vectors  # noqa: F401  (re-exported)
from trajectory_common import ALL_METHODS

pytestmark = pytest.mark.gpu

FULL = 200               # iterations of a case whose oracle stays clear of a breakdown
# transport -> (handle knobs, connect the peer exchange, schedule flags every rank must report)
TRANSPORTS = {
    'allreduce': ({'PRCG_FUSED_COMM': '0', 'PRCG_GATHER': '0'}, False, dict(comm=True, fused=False, fused_comm=False, gather=False, peer=False, window=True)),
    'two_kernel': ({'PRCG_FUSED_COMM': '0'}, False, dict(comm=True, fused=False, fused_comm=False, peer=False, window=True)),
    'gather': ({'PRCG_DEFER_GRID_PER_CU': '1', 'PRCG_FUSED_COMM': '1'}, False, dict(comm=True, fused_comm=True, gather=True, peer=False, window=True)),
    # (a grid line of 640 rows is a slot of 20 KB: beyond the 8 KB up to which a halo rides on the all-gather by default)
    'gather_32k': ({'PRCG_DEFER_GRID_PER_CU': '1', 'PRCG_FUSED_COMM': '1', 'PRCG_GATHER_MAX_BYTES': '32768'}, False,
                   dict(comm=True, fused_comm=True, gather=True, peer=False, window=True)),
    'peer': ({'PRCG_DEFER_GRID_PER_CU': '1'}, True, dict(comm=True, fused_comm=True, gather=False, peer=True, window=True)),
    # tests/test_distributed.py: test_ranks_in_threads_may_run_different_schedules -- one launch, two kernels, no window operator
    'mixed': ([{'PRCG_DEFER_GRID_PER_CU': '1', 'PRCG_FUSED_COMM': '1'}, {'PRCG_FUSED_COMM': '0'},
               {'PRCG_DEFER_GRID_PER_CU': '1', 'PRCG_FUSED_COMM': '1', 'PRCG_WIN': '0'}], False, None),
}
# operator -> (matrix, row-block offsets for R ranks or None: even)
OPERATORS = {
    's3_small': (lambda P: P.WORKLOADS['s3_small']['make'](), lambda R: None),                 # band, n = 20 000, 7-row halo
    's1_small': (lambda P: P.WORKLOADS['s1_small']['make'](), lambda R: None),                 # 64 x 48 stencil, even blocks of whole lines
    # 64 x 48 stencil cut after 3 grid lines: rank 0 has 3 tiles (one of them boundary) on one workgroup of 4 waves
    's1_uneven': (lambda P: P.WORKLOADS['s1_small']['make'](), lambda R: np.array([0, 192, 3072])),
    # 640 x 24 stencil in 3 blocks of 8 whole lines: the halo is a line of 640 rows = 10 tiles per cut
    'lap2d_640x24': (lambda P: P.laplace_2d(640, 24), lambda R: np.arange(R + 1) * 8 * 640),
}

# Jacobi is the inverse of the s3_small band to rounding (off-diagonals 1e-4): those runs reach |r| = 2e-12 at k = 4 and go on in
# rounding noise, where the Meurant flavours' predicted nu (k = 6), Ghysels-Vanroose's derived mu (k = 7) and Hestenes-Stiefel's and
# Chronopoulos-Gear's mu (k = 48) first turn non-positive under these trees -- the other flavours stay positive for 200 iterations.
BREAKS = {('pipe_pr_m_pcg', 's3_small'): 6, ('pipe_p_m_pcg', 's3_small'): 6, ('gv_pcg', 's3_small'): 7, ('hs_pcg', 's3_small'): 48, ('cg_pcg', 's3_small'): 48}


def iterations(first_bad):
    """FULL, or 10 fewer than the oracle's first state with a non-positive or non-finite mu or nu; where that state comes within the
    first 10 (which leaves no run at all) every iteration before it"""
    return FULL if first_bad < 0 else (first_bad - 10 if first_bad > 10 else first_bad - 1)


def case(method, operator, ranks, transport):
    return (method, operator, ranks, transport, iterations(BREAKS.get((method, operator), -1)))


# (method, operator, ranks, transport, iterations)
CASES = \
    [case(m + j, 's3_small', 2, t) for m in ('pipe_pr', 'pipe_p', 'pipe_pr_m', 'pipe_p_m') for j in ('_cg', '_pcg') for t in ('allreduce', 'gather', 'peer')] + \
    [case('pipe_pr' + j, 's3_small', R, 'peer') for R in (3, 4) for j in ('_cg', '_pcg')] + \
    [case(m, 'lap2d_640x24', 3, t) for m in ('pipe_pr_pcg', 'pipe_pr_m_pcg') for t in ('peer', 'gather_32k')] + \
    [case('pipe_pr_cg', 's1_uneven', 2, 'peer'), case('pipe_pr_cg', 's3_small', 3, 'mixed')] + \
    [case(m + j, 's3_small', 2, 'two_kernel') for m in ('hs', 'pr', 'cg', 'gv') for j in ('_cg', '_pcg')] + \
    [case(m, 's1_small', 3, 'two_kernel') for m in ('hs_cg', 'pr_cg')]


def case_id(c):
    return '-'.join(str(f) for f in c)


@pytest.fixture(scope='module')
def amd():
    from new_cg_variants_amd import _lib, problems
    return dict(L=_lib, problems=problems)


@pytest.fixture(scope='module')
def problem(amd):
    """operator name -> (A, b, x_true, Jacobi of the oracle, inverse diagonal), built once per module and left unchanged"""
    cache = {}

    def get(name):
        if name not in cache:
            A = OPERATORS[name][0](amd['problems'])
            b, _, x_true = amd['problems'].reference_rhs(A, A.shape[0])
            cache[name] = (A, b, x_true, orc.jacobi(A), 1 / A.diagonal())
        return cache[name]
    return get


def run_case(L, A, method, nranks, transport, offsets, inv_diag, iters, recorders, x0=None):
    knobs, peer, _ = TRANSPORTS[transport]
    return run_mode(L, A, method, nranks, knobs, peer, offsets, inv_diag, iters, recorders, x0=x0)


def pipe_tree(rank):
    """the tree of ONE rank's pipelined iteration, from the schedule it reports (module docstring)"""
    s = rank['schedule']
    if s['fused_comm']:
        assert rank['layout']['grid'] > 0 and rank['layout']['interior_grid'] == 0, rank['layout']
        return (PeerLaunchTree if s['peer'] else OneLaunchTree)(rank['layout']).sum
    assert rank['layout']['grid'] == 0, rank['layout']          # (no tile launch of the two-kernel schedule leaves partials)
    return device_sum


def oracle_dots(family, offsets, ranks):
    """(dot, dot0) for the oracle: which tree sums which inner product on every rank, in the order the oracle asks for them"""
    def every(make):
        return RankSum(offsets, [make(r) for r in ranks])
    if family == 'pipe':
        assert all(r['start_layout']['grid'] == 0 for r in ranks)
        return Routed(every(pipe_tree)), Routed(every(lambda r: device_sum))
    pair = every(lambda r: pair_sum)
    if family == 'gv':
        assert all(r['layout']['grid'] == 0 and r['start_layout']['grid'] == 0 for r in ranks)
        return Routed(pair), Routed(pair)
    assert all(r['start_layout']['grid'] > 0 and r['start_layout']['interior_grid'] == 0 for r in ranks), [r['start_layout']['grid'] for r in ranks]
    two = every(lambda r: TwoLaunchTree(r['layout']).sum)
    start = every(lambda r: OneLaunchTree(r['start_layout']).sum)
    if family == 'pr':
        return Routed(two, two, two, pair), Routed(pair, start, start, start)       # mu, delta, gamma, nu; start: nu first
    if family == 'cg':
        return Routed(two), Routed(start)                                            # nu, eta (start: then mu)
    return Routed(pair, two), Routed(pair, start)                                    # hs: nu, mu


def same_tree(a, b):
    return all(a[k] == b[k] for k in ('grid', 'waves_per_block', 'interior_grid', 'interior_waves_per_block', 'interior_tiles')) and \
        np.array_equal(a['tiles'], b['tiles'])


def shape_line(ranks):
    return ', '.join(f"{r['layout']['grid']}x{r['layout']['waves_per_block']}" +
                     (f"+{r['layout']['interior_grid']}x{r['layout']['interior_waves_per_block']}" if r['layout']['interior_grid'] else '') +
                     f" ({r['layout']['tiles'].shape[0] - r['layout']['interior_tiles']} of {r['layout']['tiles'].shape[0]} tiles boundary)" for r in ranks)


@pytest.mark.parametrize('method,operator,nranks,transport,iters', CASES, ids=[case_id(c) for c in CASES])
def test_whole_trajectory_of_a_multi_rank_session(amd, problem, method, operator, nranks, transport, iters):
    """Module docstring.  Bit for bit in both modes: every inner product the method defines and the coefficients a, b of every
    iteration on rank 0, and every rank's copy of them; one residual history; in (b) the concatenated x and r (with Jacobi r~,
    s~) at k = 3, k = 40 and the end.  The recorder histories of (a): 1e-13 relative for the three 2-norms, 1e-11 for the A-norm
    of the error (the recorder kernels sum per rank, then the all-reduce).  No wave timed out (sync() raises)."""
    whole_trajectory(amd, problem, method, operator, nranks, transport, iters)


def whole_trajectory(amd, problem, method, operator, nranks, transport, iters, x0=None):
    """the body of test_whole_trajectory_of_a_multi_rank_session.  x0: the GLOBAL start vector of every session and of the oracle
    (None: zeros).  With one, every rank's rows of x and r right after prcg_solve_begin are held first -- concatenated, x == x0 and
    r == b - A x0 with the global product, bit for bit: the halo exchange of x0 -- and the case takes no figure from BREAKS: it
    runs `iters` iterations and asserts that the oracle's mu and nu are finite and positive at every one of them."""
    L = amd['L']
    variant, family, jac, slots = ALL_METHODS[method]
    A, b, x_true, jacobi, inv_diag = problem(operator)
    off = OPERATORS[operator][1](nranks)
    runs = [run_case(L, A, method, nranks, transport, off, inv_diag, iters, rec, x0=x0) for rec in (True, False)]
    offsets = runs[0][0]
    assert np.array_equal(offsets, runs[1][0])
    flags = TRANSPORTS[transport][2]
    for mode, (_, ranks) in zip('ab', runs):
        scheds = [r['schedule'] for r in ranks]
        if transport == 'mixed':
            assert [s['fused_comm'] for s in scheds] == [True, False, False] and all(s['comm'] and s['gather'] and not s['peer'] for s in scheds), (mode, scheds)
            assert [s['window'] for s in scheds] == [True, True, False], (mode, scheds)
        else:
            assert all(s[k] == v for s in scheds for k, v in flags.items()), (mode, flags, scheds)
    # the branches the case is there for, from the layouts
    lays = [r['layout'] for r in runs[0][1]]
    bnd = [lay['tiles'].shape[0] - lay['interior_tiles'] for lay in lays]
    if operator == 's3_small' and transport != 'mixed':
        assert all(0 < x <= 8 for x in bnd), bnd                   # the communication wave of the peer exchange takes them
    if operator == 'lap2d_640x24':
        assert max(bnd) > 8, bnd                                   # they stay with all the waves
    if operator == 's1_uneven':
        assert lays[0]['tiles'].shape[0] < lays[0]['grid'] * lays[0]['waves_per_block'] and 0 < bnd[0] <= 8, (lays[0]['tiles'].shape, bnd)
    hold_ranks_to_oracle(L, case_id((method, operator, nranks, transport, iters)), method, A, b, x_true, jacobi, runs,
                         oracle_dots(family, offsets, runs[0][1]), iters, FULL, iterations, same_tree, shape_line, x0=x0)
