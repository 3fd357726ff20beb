"""A used handle opens every session exactly as a fresh one does (csrc/prcg_session.cpp: open_session resets the whole
Session in one place).  cg_variants caches operators so that all nine variants run on ONE handle; here a handle runs a
sequence of sessions of every family, and each is compared -- on the 64-bit patterns, as tests/test_xp_deferred.py does --
with the same session on a handle that has never run anything else: every state vector the session serves, the scalars of
iterations 0..12, the coefficients of 1..12, the histories and the whole schedule() dict."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MAX_ITER = 13
CALLS = (5, 7)
KNOBS = {'PRCG_SMALL': '0'}


@pytest.fixture(scope='module')
def amd():
    from new_cg_variants_amd import _lib, device, problems
    A = problems.WORKLOADS['s3_small']['make']()          # ex2b band, n = 20,000: a window operator
    n = A.shape[0]
    b, x0, _ = problems.reference_rhs(A, n)
    rng = np.random.default_rng(5)
    B = np.stack([b, rng.standard_normal(n)])
    X0 = np.stack([x0, rng.standard_normal(n)])
    inv_diag = 1 / A.diagonal()
    # point-block Jacobi, 2 x 2: inverses of the diagonal blocks
    d, up, lo = A.diagonal(), A.diagonal(1)[::2], A.diagonal(-1)[::2]
    blocks = np.empty((n // 2, 2, 2))
    blocks[:, 0, 0], blocks[:, 1, 1], blocks[:, 0, 1], blocks[:, 1, 0] = d[0::2], d[1::2], up, lo
    return dict(L=_lib, device=device, A=A, n=n, b=b, x0=x0, B=B, X0=X0, inv_diag=inv_diag, inv_blocks=np.linalg.inv(blocks))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# (label, variant, two right-hand sides, preconditioner: None | 'jacobi' | 'block', clear_preconditioners afterwards)
SESSIONS = [
    ('cg_cg', 'CG_CG', False, None, False),
    ('pipe_pr', 'PIPE_PR', False, None, False),
    ('hs x2', 'HS', True, None, False),
    ('gv', 'GV', False, None, False),
    ('pr jacobi', 'PR', False, 'jacobi', False),
    ('hs jacobi', 'HS', False, 'jacobi', False),
    ('pipe_p_m jacobi', 'PIPE_P_M', False, 'jacobi', False),
    ('cg_cg jacobi', 'CG_CG', False, 'jacobi', False),
    ('hs block jacobi', 'HS', False, 'block', True),
    ('hs', 'HS', False, None, False),
    ('hs x2 jacobi', 'HS', True, 'jacobi', False),
]


def run_session(amd, op, session, extra_hist):
    """Open the session on `op`, run it, and return everything a caller can read of it."""
    L = amd['L']
    _, variant, rhs2, prec, clear = session
    hist = L.HIST_UPDATED_RESIDUAL_2_NORM | (0 if rhs2 else extra_hist)      # (the two-RHS session serves the recurrence residual only)
    inv_diag = amd['inv_diag'] if prec == 'jacobi' else None
    if rhs2:
        op.begin_multi(getattr(L, variant), amd['B'], amd['X0'], MAX_ITER, inv_diag=inv_diag, hist_mask=hist)
    else:
        op.begin(getattr(L, variant), amd['b'], amd['x0'], MAX_ITER, inv_diag=inv_diag, hist_mask=hist,
                 block_jacobi=(2, amd['inv_blocks']) if prec == 'block' else None)
    out = {'schedule@begin': op.schedule()}
    for call in CALLS:
        op.iterate(call)
    assert op.k == sum(CALLS) == MAX_ITER - 1
    out['schedule'] = op.schedule()
    for j in ((0, 1) if rhs2 else (None,)):
        tag = '' if j is None else f'[{j}]'
        for name in L.VEC:
            try:
                out[f'vector {name}{tag}'] = op.get_vector(name, rhs=j)
            except L.PrcgError:
                out[f'vector {name}{tag}'] = None                         # not part of this session: on both handles or on neither
        for k in range(MAX_ITER):
            out[f'scalars {k}{tag}'] = op.get_scalars(k, rhs=j)
        for k in range(1, MAX_ITER):
            out[f'coefficients {k}{tag}'] = op.get_coefficients(k, rhs=j)
        for q, v in op.history(rhs=j).items():
            out[f'history {q}{tag}'] = v
    if clear:
        op.clear_preconditioners()
    return out


def assert_same_session(label, used, fresh):
    assert used.keys() == fresh.keys(), label
    for key in used:
        if key.startswith('schedule'):
            assert used[key] == fresh[key], (label, key, {f: (used[key][f], fresh[key][f]) for f in used[key] if used[key][f] != fresh[key][f]})
        elif used[key] is None or fresh[key] is None:
            assert used[key] is None and fresh[key] is None, (label, key)
        else:
            assert same_bits(used[key], fresh[key]), (label, key)
    assert sum(v is not None for k, v in used.items() if k.startswith('vector')) >= 4, label


@pytest.mark.parametrize('true_residual', [False, True])
def test_used_handle_runs_every_session_as_a_fresh_one(amd, true_residual):
    """One handle, eleven sessions of all four families in a row; true_residual adds HIST_RESIDUAL_2_NORM where the session
    serves it, so that record()'s flushes run after every iteration."""
    extra = amd['L'].HIST_RESIDUAL_2_NORM if true_residual else 0
    used = amd['device'].DeviceCSR(amd['A'], knobs=KNOBS)
    for session in SESSIONS:
        got = run_session(amd, used, session, extra)
        fresh = amd['device'].DeviceCSR(amd['A'], knobs=KNOBS)
        want = run_session(amd, fresh, session, extra)
        fresh.close()
        assert_same_session(session[0], got, want)
    used.close()


def test_used_handle_with_a_communicator(amd):
    """The same with a one-rank communicator and PRCG_FUSED_COMM=1: after a one-launch communicator session the
    Hestenes-Stiefel and Chronopoulos-Gear sessions report -- and run -- what they do on a fresh handle; in particular no
    FUSED_COMM / PEER flag is left over from the pipelined session before them."""
    from test_distributed import rccl_ids
    knobs = dict(KNOBS, PRCG_FUSED_COMM='1')

    def handle():
        uid, path = rccl_ids(1)                       # a new id per handle
        return amd['device'].DeviceCSR(amd['A'], comm_init=(0, 1, uid, path), knobs=knobs)

    sessions = [(label, variant, False, None, False)
                for label, variant in (('pipe_pr', 'PIPE_PR'), ('hs', 'HS'), ('cg_cg', 'CG_CG'), ('pipe_pr again', 'PIPE_PR'))]
    # one handle open at a time (its three streams then map to hardware queues of their own, which the one-launch
    # communicator schedule probes for at session start): the fresh handles first, then the used one
    wants = []
    for session in sessions:
        fresh = handle()
        wants.append(run_session(amd, fresh, session, 0))
        fresh.close()
    used = handle()
    for session, want in zip(sessions, wants):
        label, variant = session[:2]
        got = run_session(amd, used, session, 0)
        for key in ('schedule@begin', 'schedule'):
            assert got[key]['comm'] and want[key]['comm'], (label, key)
            assert got[key]['fused_comm'] == want[key]['fused_comm'] and got[key]['peer'] == want[key]['peer'], (label, key, got[key], want[key])
            if variant in ('HS', 'CG_CG'):
                assert not got[key]['fused_comm'] and not got[key]['peer'], (label, key, got[key])
        assert_same_session(label, got, want)
    used.close()
