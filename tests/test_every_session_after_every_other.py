"""ONE DeviceCSR handle runs every kind of session right after every other kind -- all K * K ordered pairs, self-pairs included,
each exactly once (tests/handle_walk_common.py: an Euler circuit of K * K + 1 runs) -- and every run is compared, on the 64-bit
patterns, with the same kind's run on a handle that has never run anything else.  The fresh handle is the reference; each kind is
held to the device-ordered oracle on a fresh handle by the module the table names, so equal bits here carry that to a used handle.
tests/test_session_reuse.py (one list of eleven sessions) and tests/test_stop_kinds_share_a_handle.py (six kinds forwards and
backwards) look at 11 pairs each; a leak shows for ONE ordered pair, "B right after A".

Operators, the smallest that take every product path (all but nos7 with PRCG_SMALL=0):
  s3_small     banded_ex2b(20000, 7): window tiles with a value dictionary; n = 20 000 = 6666 * 3 + 2, a short last 3 x 3 block
  fem12        fem_like_3d(12), n = 5184: sliced rows, the one-launch four-vector product
  fem12_csr    the same matrix with PRCG_SELL=0: CSR-adaptive tiles
  nos7         golden, n = 729, default knobs: the one-workgroup solver serves hs, pipe_pr and pipe_pr_stop, the general path (window
               tiles) every other kind ON THE SAME HANDLE.  begin refuses no kind there: none is dropped on any operator.

Run shape: max_iter = 13, iterate(5); iterate(7) without a sync between them (tests/test_session_reuse.py's): partials stay
pending across a call boundary and the deferred (x,p) store sees both parities; x0 = 0; the recurrence residual recorded.

Kinds (K = 23).  Every recipe is self-contained: a single session sets or clears the replace hook itself, the multi begins call
clear_preconditioners() and set_replace_hook(None) first, as cg_variants does (begin_multi* refuse a handle that has them: the
documented contract).  Right-hand sides: b = A @ default_rng(7).standard_normal(n) for the single sessions, column c = A @
default_rng(8 + c).standard_normal(n) for the multi sessions -- their column 0 is NOT b: a two-RHS pipe_pr session with inv_diag and
a single pipe_pr session with the callback v -> d * v are the same computation summed in the same order (both device_dot's), and end
at the same x bit for bit on the same right-hand side, which is no leak and tells nothing -- under these the
recurrence residual of every oracle run falls from row to row on all four operators, so a threshold taken from a middle row
stops the run inside it (with b = A @ const, the reference's, r.r of the unpreconditioned runs on fem12 and nos7 never falls
below its first value within 13 iterations: no threshold on r.r would stop them after their start).
  kind                  session                                                          held to the oracle on a fresh handle by
  hs                    begin(HS)                                                        test_trajectory_oracle / _irregular
  hs_jacobi_stop        begin(HS, inv_diag, rr_stop)                                     test_hs_stop
  cg_cg_jacobi          begin(CG_CG, inv_diag)                                           test_trajectory_oracle / _irregular
  gv                    begin(GV)                                                        test_trajectory_oracle / _irregular
  gv_replace            begin(GV), replace hook firing at k % 3 == 0                     test_gpu_parity (w_replace: within 1e-11 of the
                                                                                         reference, not bit for bit -- the one kind here
                                                                                         whose own module holds it with a tolerance)
  pr                    begin(PR)                                                        test_trajectory_oracle / _irregular
  m_jacobi              begin(M, inv_diag)                                               test_trajectory_oracle / _irregular
  pipe_pr               begin(PIPE_PR)                                                   test_trajectory_oracle / _irregular
  pipe_p_m_jacobi       begin(PIPE_P_M, inv_diag)                                        test_trajectory_oracle / _irregular
  pipe_pr_stop          begin(PIPE_PR, rr_stop)                                          test_single_stop
  pipe_pr_callback      begin(PIPE_PR, preconditioner = v -> d * v on the host)          test_trajectory_stored_tilde
  hs_built3             begin(HS, block_jacobi=(3, None)): built on the device           test_trajectory_stored_tilde, test_block_jacobi_build
  pipe_p_bj3_stop       begin(PIPE_P, block_jacobi=(3, H), rr_stop)                      test_block_jacobi_stop
  pr_built_var          begin(PR, block_jacobi_var=(cyclic 1..8, None))                  test_trajectory_stored_tilde, test_block_jacobi_var
  cg_cg_var             begin(CG_CG, block_jacobi_var=(cyclic 1..8, Hv))                 test_trajectory_stored_tilde
  multi_hs2             begin_multi(HS, 2 columns)                                       test_multi_rhs
  multi_pr4_jacobi      begin_multi(PR, 4 columns, inv_diag)                             test_multi_rhs4
  multi_pipe_jacobi     begin_multi_pipe(PIPE_PR, inv_diag)                              test_multi_rhs_pipe
  multi_pipe_m_stop     begin_multi_pipe(PIPE_PR_M, rr_stop=[t0, t1])                    test_multi_rhs_stop
  multi_hs4_built3      begin_multi_block_jacobi(HS, 4 columns, block_jacobi=(3, None))  test_multi_rhs_block_jacobi
  multi_pr2_var         begin_multi_block_jacobi(PR, 2 columns, block_jacobi_var=(.., Hv)) test_multi_rhs_block_jacobi
  products              matvec, matmat2, matmat4 of fixed inputs (they share tmp_ext /   test_gpu_parity, test_row_walk, test_multi_rhs4
                        t1 / x4b / y4b with the sessions); no session
  same_values           update_values(A.data), then matvec: no bit may change, and a     test_update_values
                        later "built" kind must rebuild to the same bits
H, Hv: LAPACK inverses of the blocks of A + 0.5 diag(A) -- NOT the blocks the device builds from A, so a stale _bj_built /
_bjv_built or a stale block table on the handle changes bits.

Compared per run: schedule() after begin and at the end, every vector of L.VEC (None where the session does not serve it, on
both handles or on neither), scalars of rows 0..12, coefficients of rows 1..12, every history, stop() / stops_rhs(), k; per
column for the multi sessions; the products of the two kinds without a session.

Thresholds, all from the oracle on the CPU (setup(), asserted without a GPU), as tests/test_stop_kinds_share_a_handle.plan()
derives them: pipe_p_bj3_stop and multi_pipe_m_stop run two-kernel schedules that device_order.device_dot restates exactly: thr =
rr of an oracle row (row 6, on s3_small row 3: BJ_ROW; rows 4 and 8 of the two columns).  hs_jacobi_stop and pipe_pr_stop sum in an order that depends on
the launch: thr = the geometric mean of rr at k and k - 1, k the first row with rr <= rr[6], every earlier rr above thr and rr[k]
below it by more than one part in 1000.  The stop found on the fresh handle must equal the plan.

Two passes per operator: `read` -- every session run to its end and read; `abandoned` -- after the compared run the same kind is
begun AGAIN, iterate(3) is called and nothing else, no sync, no read-out, and the next kind begins: every pair also with a
predecessor that left partials, a deferred store, a packed state, a lagging update or an armed stop word behind.  Each pass
compares K * K + 1 = 530 runs, asserted.

Measured on an MI355X (every pair equal on every operator in both passes): the eight cases take 0.9 to 2.1 s each, 10.8 s together
-- s3_small 2.1 s (read, with its 23 fresh handles: 0.8 s) and 1.3 s (abandoned), fem12 1.6 / 1.1 s, fem12_csr 1.3 / 1.0 s, nos7
1.2 / 0.9 s: about 2 ms per run, begin and read-out included, so no case is cut into segments (handle_walk_common.segments)."""
import functools

import numpy as np
import pytest

import block_jacobi_stop_common as bjc
import handle_walk_common as hw
import hs_stop_common as hsc
import multi_rhs_stop_common as rhsc
import single_stop_common as ssc
import test_multi_rhs_pipe as pipe
from device_order import device_dot
from test_stop_kinds_share_a_handle import between_rows

MAX_ITER = 13
CALLS = (5, 7)
ROW = MAX_ITER // 2
RHS_ROWS = (4, 8)
# the oracle row whose rr is pipe_p_bj3_stop's threshold.  s3_small: under these blocks the band reaches the accuracy it can attain at
# row 4 and the oracle's mu turns non-positive at row 5 -- the rule would report a breakdown before rr[6] is met -- so row 3 there
BJ_ROW = {'s3_small': 3}
# operator -> (matrix, knobs of the handle, the product family its schedule() reports)
OPERATORS = {'s3_small': ('s3_small', {'PRCG_SMALL': '0'}, 'window'), 'fem12': ('fem12', {'PRCG_SMALL': '0'}, 'sliced'),
             'fem12_csr': ('fem12', {'PRCG_SMALL': '0', 'PRCG_SELL': '0'}, 'csr'), 'nos7': ('nos7', {}, 'window')}
PASSES = ('read', 'abandoned')

# kind -> its recipe.  how: 'single' (begin), 'multi' / 'multi_pipe' / 'multi_blocks' (the three multi begins), 'products', 'values'
KINDS = {
    'hs': dict(how='single', variant='HS'),
    'hs_jacobi_stop': dict(how='single', variant='HS', jacobi=True, stop='hs_thr'),
    'cg_cg_jacobi': dict(how='single', variant='CG_CG', jacobi=True),
    'gv': dict(how='single', variant='GV'),
    'gv_replace': dict(how='single', variant='GV', replace=True),
    'pr': dict(how='single', variant='PR'),
    'm_jacobi': dict(how='single', variant='M', jacobi=True),
    'pipe_pr': dict(how='single', variant='PIPE_PR'),
    'pipe_p_m_jacobi': dict(how='single', variant='PIPE_P_M', jacobi=True),
    'pipe_pr_stop': dict(how='single', variant='PIPE_PR', stop='pipe_thr'),
    'pipe_pr_callback': dict(how='single', variant='PIPE_PR', callback=True),
    'hs_built3': dict(how='single', variant='HS', bj='built'),
    'pipe_p_bj3_stop': dict(how='single', variant='PIPE_P', bj='host', stop='bj_thr'),
    'pr_built_var': dict(how='single', variant='PR', bjv='built'),
    'cg_cg_var': dict(how='single', variant='CG_CG', bjv='host'),
    'multi_hs2': dict(how='multi', variant='HS', nrhs=2),
    'multi_pr4_jacobi': dict(how='multi', variant='PR', nrhs=4, jacobi=True),
    'multi_pipe_jacobi': dict(how='multi_pipe', variant='PIPE_PR', nrhs=2, jacobi=True),
    'multi_pipe_m_stop': dict(how='multi_pipe', variant='PIPE_PR_M', nrhs=2, stop='rhs_thr'),
    'multi_hs4_built3': dict(how='multi_blocks', variant='HS', nrhs=4, bj='built'),
    'multi_pr2_var': dict(how='multi_blocks', variant='PR', nrhs=2, bjv='host'),
    'products': dict(how='products'),
    'same_values': dict(how='values'),
}
NO_SESSION = ('products', 'same_values')
STOPPING = {'hs_jacobi_stop': 'hs_stop', 'pipe_pr_stop': 'pipe_stop', 'pipe_p_bj3_stop': 'bj_stop'}
# the one-workgroup solver's kinds on the nos7 handle (unpreconditioned HS / PIPE_PR, the recurrence residual only)
SMALL_ON_NOS7 = ('hs', 'pipe_pr', 'pipe_pr_stop')


@functools.lru_cache(maxsize=None)
def setup(name):
    """Everything the sessions of one operator need, from the CPU alone, computed once and left unchanged: the system, the host
    inverses of the shifted matrix, the inputs of the products, the thresholds and where the oracle stops under them"""
    import scipy.sparse as sp
    import new_cg_variants_amd.cg_variants as cgv
    from new_cg_variants_amd import problems as P
    matrix = OPERATORS[name][0]
    if matrix == 'nos7':
        from conftest import load_matrix
        A = load_matrix('nos7')[0]
    else:
        A = sp.csr_matrix(P.WORKLOADS['s3_small']['make']() if matrix == 's3_small' else P.fem_like_3d(12))
    n = A.shape[0]
    b = A @ np.random.default_rng(7).standard_normal(n)
    B4 = np.stack([A @ np.random.default_rng(s).standard_normal(n) for s in (8, 9, 10, 11)])
    shifted = sp.csr_matrix(A + 0.5 * sp.diags(A.diagonal()))
    ptr = bjc.cyclic_partition(n)
    host3, hostv = cgv.BlockJacobi(shifted, 3), cgv.VarBlockJacobi(shifted, ptr)
    S = dict(A=A, n=n, b=b, x0=np.zeros(n), B2=B4[:2].copy(), B4=B4, inv_diag=1 / A.diagonal(),
             ptr=ptr, bj_host=host3.inv_blocks, bjv_host=hostv.inv_blocks,
             px=np.random.default_rng(21).standard_normal(n), px2=np.random.default_rng(22).standard_normal((n, 2)),
             px4=np.random.default_rng(23).standard_normal((n, 4)))
    iters = MAX_ITER - 1
    with np.errstate(all='ignore'):
        traj = hsc.trajectory_np(A, b, 'hs_pcg', iters, keep=())
        S['hs_thr'], k = between_rows(traj['scalars'][:, 4], ROW)
        S['hs_stop'] = hsc.stop_of(traj, S['hs_thr'])
        assert S['hs_stop'] == (k, ssc.CONVERGED)
        traj = ssc.trajectory(A, b, 'pipe_pr_cg', device_dot, device_dot, iters, keep=())
        S['pipe_thr'], k = between_rows(traj['scalars'][:, 4], ROW)
        S['pipe_stop'] = ssc.stop_of(traj, S['pipe_thr'])
        assert S['pipe_stop'] == (k, ssc.CONVERGED)
        traj = bjc.trajectory(A, b, 'PIPE_P', host3, iters)
        S['bj_thr'] = float(traj['scalars'][BJ_ROW.get(name, ROW), 4])
        S['bj_stop'] = ssc.stop_of(traj, S['bj_thr'])
        rows = [pipe.oracle_column(A, S['B2'][c], S['x0'], iters, False, 'pr_m')['scalars'] for c in range(2)]
        S['rhs_thr'] = [float(rows[c][RHS_ROWS[c], 4]) for c in range(2)]
        S['rhs_stops'] = [rhsc.stop_of(rows[c], S['rhs_thr'][c]) for c in range(2)]
        S['rhs_finite'] = bool(np.isfinite(rows[0]).all() and np.isfinite(rows[1]).all())
    for v in S.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return S


@pytest.mark.parametrize('name', list(OPERATORS))
def test_the_plan_stops_every_stopping_kind_strictly_inside_its_run(name):
    """no GPU: every threshold is positive and the oracle stops under it converged, after its start and before the run's last
    iteration; the two columns of the two-RHS session at different iterations (between_rows asserts the margins of the two
    order-dependent kinds, setup that their rule fires at the k between_rows found)"""
    S = setup(name)
    for key in ('hs', 'pipe', 'bj'):
        k, status = S[f'{key}_stop']
        assert status == ssc.CONVERGED and 0 < k < MAX_ITER - 1 and S[f'{key}_thr'] > 0, (name, key, S[f'{key}_stop'], S[f'{key}_thr'])
    (k0, s0), (k1, s1) = S['rhs_stops']
    assert s0 == s1 == ssc.CONVERGED and 0 < k0 < MAX_ITER - 1 and 0 < k1 < MAX_ITER - 1 and k0 != k1, (name, S['rhs_stops'])
    assert min(S['rhs_thr']) > 0 and S['rhs_finite']
    assert len(KINDS) == 23 and len(hw.all_pairs_sequence(len(KINDS))) == 530


def begin(kind, L, op, S):
    """open the session of `kind` on op (the kinds without a session have none to open)"""
    t = KINDS[kind]
    variant = getattr(L, t['variant'])
    blocks = {}
    if 'bj' in t:
        blocks['block_jacobi'] = (3, S['bj_host'] if t['bj'] == 'host' else None)
    if 'bjv' in t:
        blocks['block_jacobi_var'] = (S['ptr'], S['bjv_host'] if t['bjv'] == 'host' else None)
    inv_diag = S['inv_diag'] if t.get('jacobi') else None
    rr_stop = S[t['stop']] if 'stop' in t else None
    if t['how'] == 'single':
        op.set_replace_hook((lambda k: k % 3 == 0) if t.get('replace') else None)
        d = S['inv_diag']
        op.begin(variant, S['b'], S['x0'], MAX_ITER, inv_diag=inv_diag, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM, rr_stop=rr_stop,
                 preconditioner=(lambda v: d * v) if t.get('callback') else None, **blocks)
        return
    op.clear_preconditioners()
    op.set_replace_hook(None)
    B = S['B2'] if t['nrhs'] == 2 else S['B4']
    X0 = np.zeros(B.shape)
    if t['how'] == 'multi':
        op.begin_multi(variant, B, X0, MAX_ITER, inv_diag=inv_diag, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM)
    elif t['how'] == 'multi_pipe':
        op.begin_multi_pipe(variant, B, X0, MAX_ITER, inv_diag=inv_diag, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM, rr_stop=rr_stop)
    else:
        op.begin_multi_block_jacobi(variant, B, X0, MAX_ITER, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM, **blocks)


def read_column(L, op, j):
    """everything a caller can read of the open session (j: of its column j), as tests/test_session_reuse.py reads it"""
    at = {}
    for v in L.VEC:
        try:
            at[v] = op.get_vector(v, rhs=j)
        except L.PrcgError:
            at[v] = None                       # not part of this session: on both handles or on neither
    return dict(at=at, scalars=np.array([op.get_scalars(k, rhs=j) for k in range(MAX_ITER)]),
                coef=np.array([op.get_coefficients(k, rhs=j) for k in range(1, MAX_ITER)]), hist=op.history(rhs=j))


def run(kind, L, op, S):
    """one run of `kind` on op, read back in full"""
    t = KINDS[kind]
    if t['how'] == 'products':
        return dict(y=op.matvec(S['px'])[0], wu=op.matmat2(S['px2'])[0], y4=op.matmat4(S['px4'])[0])
    if t['how'] == 'values':
        return dict(route=op.update_values(S['A'].data), y=op.matvec(S['px'])[0])
    begin(kind, L, op, S)
    out = {'schedule@begin': op.schedule()}
    for c in CALLS:
        op.iterate(c)
    if t['how'] == 'single':
        out.update(read_column(L, op, None), stop=op.stop())
    else:
        out.update(cols=[read_column(L, op, j) for j in range(t['nrhs'])], stops=op.stops_rhs())
    out.update(k=int(op.k), schedule=op.schedule())
    return out


def abandon(kind, L, op, S):
    """the same kind begun again and left mid-run: three iterations queued, no sync, nothing read"""
    if kind not in NO_SESSION:
        begin(kind, L, op, S)
        op.iterate(3)


def leaves(rec, path=''):
    if isinstance(rec, dict):
        for key, v in rec.items():
            yield from leaves(v, f'{path}/{key}')
    elif isinstance(rec, (list, tuple)):
        for i, v in enumerate(rec):
            yield from leaves(v, f'{path}[{i}]')
    elif rec is not None and not isinstance(rec, (str, bool)):
        yield path, np.asarray(rec)


def check_fresh(name, fresh, S):
    """non-vacuity, on the reference runs: everything finite, every schedule what the table claims, distinct kinds distinct bits,
    every stopping kind stopped where the plan says and every other kind ran to its end"""
    family = OPERATORS[name][2]
    for kind, rec in fresh.items():
        bad = [path for path, v in leaves(rec) if v.dtype.kind == 'f' and not np.isfinite(v).all()]
        assert not bad, (name, kind, 'not finite', bad[:6])
        if kind in NO_SESSION:
            assert np.array_equal(rec['y'], S['A'] @ S['px']), (name, kind, 'the product is SciPy\'s, bit for bit')
            assert kind == 'products' or rec['route'] in ('in_place', 'replanned'), rec['route']
            continue
        t = KINDS[kind]
        for s in (rec['schedule@begin'], rec['schedule']):
            what = (name, kind, s)
            assert s['window'] == (family == 'window') and s['sliced_rows'] == (family == 'sliced'), what
            assert (s['value_dict'] or name != 's3_small') and not s['comm'] and not s['fused_comm'] and not s['peer'], what
            assert s['small'] == (name == 'nos7' and kind in SMALL_ON_NOS7), what
            assert s['block_jacobi'] == ('bj' in t or 'bjv' in t) and s['block_jacobi_var'] == ('bjv' in t), what
            nrhs = t.get('nrhs', 1)
            assert s['rhs2'] == (nrhs == 2) and s['rhs4'] == (nrhs == 4) and s['rhs2_pipe'] == (t['how'] == 'multi_pipe'), what
            assert s['spmm4'] == (family == 'sliced' and (nrhs == 4 or t['how'] == 'multi_pipe')), what
            if t['how'] == 'single' and t['variant'] in ('HS', 'PIPE_PR', 'PIPE_P_M'):
                stored_tilde = 'bj' in t or 'bjv' in t or t.get('callback')
                assert s['fused'] == (not stored_tilde), what           # one launch per iteration; none with a stored r~, s~, ..
            # the deferred (x,p) store: one-launch pipelined sessions on window tiles -- not the one-workgroup solver, and not with
            # a threshold, where every launch closes itself
            deferred = t['how'] == 'single' and t['variant'].startswith('PIPE') and s['fused'] and family == 'window' and not s['small']
            assert s['xp_deferred'] == (deferred and 'stop' not in t), what
        served = [v for col in (rec['cols'] if 'cols' in rec else [rec]) for v in col['at'].values() if v is not None]
        assert len(served) >= 4 * t.get('nrhs', 1), (name, kind, 'vectors served')
        if kind in STOPPING:
            assert rec['stop'] == S[STOPPING[kind]] and rec['k'] == rec['stop'][0], (name, kind, rec['stop'], rec['k'], S[STOPPING[kind]])
        elif kind == 'multi_pipe_m_stop':
            assert rec['stops'] == S['rhs_stops'] and rec['k'] == max(k for k, _ in S['rhs_stops']), (name, kind, rec['stops'], rec['k'])
        elif t['how'] == 'single':
            assert rec['stop'] == (-1, 0) and rec['k'] == MAX_ITER - 1, (name, kind, rec['stop'], rec['k'])
        else:
            assert rec['stops'] == [(-1, 0)] * t['nrhs'] and rec['k'] == MAX_ITER - 1, (name, kind, rec['stops'], rec['k'])
    # the same right-hand side -- b of every single session, column 0 of every multi session -- and no two kinds the same x
    for group in ([k for k in fresh if 'cols' not in fresh[k] and k not in NO_SESSION], [k for k in fresh if 'cols' in fresh[k]]):
        xs = {kind: (fresh[kind]['cols'][0] if 'cols' in fresh[kind] else fresh[kind])['at']['x'] for kind in group}
        same = [(a, b) for i, a in enumerate(group) for b in group[i + 1:] if np.array_equal(xs[a], xs[b])]
        assert len(group) >= 6 and not same, (name, 'kinds that end at the same x bit for bit', same)


_fresh = {}


def fresh_runs(name, L, device):
    """kind -> its run on a handle that has run nothing else: the reference of both passes, computed once, checked, left unchanged"""
    if name not in _fresh:
        S = setup(name)
        recs = {}
        for kind in KINDS:
            op = device.DeviceCSR(S['A'], knobs=dict(OPERATORS[name][1]))
            try:
                recs[kind] = run(kind, L, op, S)
            finally:
                op.close()
        check_fresh(name, recs, S)
        _fresh[name] = recs
    return _fresh[name]


@pytest.mark.gpu
@pytest.mark.parametrize('how', PASSES)
@pytest.mark.parametrize('name', list(OPERATORS))
def test_every_kind_after_every_other_equals_a_fresh_handle(name, how):
    import time
    from new_cg_variants_amd import _lib as L
    from new_cg_variants_amd import device
    S = setup(name)
    t0 = time.perf_counter()
    fresh = fresh_runs(name, L, device)
    t1 = time.perf_counter()
    op = device.DeviceCSR(S['A'], knobs=dict(OPERATORS[name][1]))
    try:
        got = hw.walk(list(KINDS), lambda kind: run(kind, L, op, S), fresh,
                      leave=(lambda kind: abandon(kind, L, op, S)) if how == 'abandoned' else None)
    finally:
        op.close()
    K = len(KINDS)
    print(f'{name} {how}: {got.compared} runs compared, {len(got.found)} differ; fresh handles {t1 - t0:.2f} s, walk {time.perf_counter() - t1:.2f} s')
    assert got.compared == K * K + 1 == 530
    pairs = set(zip(got.sequence, got.sequence[1:]))
    assert len(pairs) == K * K, 'every ordered pair of kinds was consecutive on the walked handle'
    assert not got.found, f'{name}, pass {how}:\n' + hw.render(list(KINDS), got.found)
