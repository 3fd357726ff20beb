"""Deferred (x,p) store of the single-GPU one-launch pipelined iteration.

A qualifying session runs the launches of one prcg_iterate call as (SKIP, APPLY) pairs: the first launch of a pair does not
store (x,p), the second rebuilds them from the unchanged pair in memory, the row's own r (r~) and the skipped iteration's
stored a, b -- the same operands and expressions, so NO rounding changes.  Every comparison here is therefore bitwise
(on the 64-bit patterns, so that a NaN would have to match too)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def amd():
    from new_cg_variants_amd import _lib, device, problems
    return dict(L=_lib, device=device, problems=problems)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def make_operator(P, source):
    if source == 'band':
        return P.WORKLOADS['s3_small']['make']()         # ex2b band, 15 diagonals: 1-byte window indices
    if source == 'lap3d':
        return P.laplace_3d(24, 20, 18)                  # a grid plane of 480 rows: 2-byte window indices, or pattern tiles
    if source == 'lap2d':
        return P.laplace_2d(130, 77)                     # pattern tiles of a 2-D stencil
    raise KeyError(source)


# operator, knobs, expected encodings (bytes per window index or None, value dictionary or None, pattern tiles)
OPERATORS = [
    ('band', {}, 1, True, False),
    ('band', {'PRCG_VALDICT': '0'}, 1, False, False),
    ('lap3d', {'PRCG_WIN_PAT': '0'}, 2, None, False),
    ('lap3d', {'PRCG_WIN_PAT': '0', 'PRCG_VALDICT': '0'}, 2, False, False),
    ('lap2d', {}, None, True, True),
    ('lap3d', {}, None, True, True),
]
CALLS = (1, 2, 3, 7, 40, 3, 1, 2)       # lengths 1, 2, 3, 7 and 40 mixed in one session: odd and even, pairs and remainders


@pytest.mark.parametrize('jacobi', [False, True])
@pytest.mark.parametrize('variant', ['PIPE_PR', 'PIPE_P', 'PIPE_PR_M', 'PIPE_P_M'])
@pytest.mark.parametrize('source,knobs,col_bytes,value_dict,pattern', OPERATORS)
def test_deferred_store_changes_no_bit(amd, source, knobs, col_bytes, value_dict, pattern, variant, jacobi):
    """The same free-running session with PRCG_XP_DEFER=1 and 0: after every prcg_iterate call x, p, r, s (r~, s~ with
    Jacobi, the stored w, w~ of the 'p' flavours), every stored scalar and every coefficient are equal bit for bit."""
    L, P = amd['L'], amd['problems']
    A = make_operator(P, source)
    n = A.shape[0]
    b, x0, _ = P.reference_rhs(A, n)
    inv_diag = (1 / A.diagonal()) if jacobi else None
    ops = [amd['device'].DeviceCSR(A, knobs=dict(knobs, PRCG_SMALL='0', PRCG_XP_DEFER=d)) for d in ('1', '0')]
    total = sum(CALLS)
    for op in ops:
        op.begin(getattr(L, variant), b, x0, total + 1, inv_diag=inv_diag, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM)
        s = op.schedule()
        assert s['fused'] and s['window'] and not s['small'] and s['pattern'] == pattern, s
        if col_bytes is not None:
            assert s['col_bytes'] == col_bytes, s
        if value_dict is not None:
            assert s['value_dict'] == value_dict, s
    assert ops[0].schedule()['xp_deferred'] and not ops[1].schedule()['xp_deferred']
    vectors = ['x', 'p', 'r', 's'] + (['rt', 'st'] if jacobi else [])
    if variant in ('PIPE_P', 'PIPE_P_M'):
        vectors += ['w'] + (['wt'] if jacobi else [])
    k = 0
    for call in CALLS:
        for op in ops:
            op.iterate(call)
        for v in vectors:
            assert same_bits(ops[0].get_vector(v), ops[1].get_vector(v)), (k, call, v)
        for kk in range(k, k + call + 1):
            assert same_bits(ops[0].get_scalars(kk), ops[1].get_scalars(kk)), (k, call, kk)
        for kk in range(k + 1, k + call + 1):
            assert same_bits(ops[0].get_coefficients(kk), ops[1].get_coefficients(kk)), (k, call, kk)
        k += call
    assert ops[0].k == total and ops[1].k == total
    h0, h1 = ops[0].history(), ops[1].history()
    for q in h0:
        assert same_bits(h0[q], h1[q]), q
    for op in ops:
        op.close()


def test_which_sessions_defer(amd):
    """xp_deferred is reported by qualifying sessions only: single GPU, window operator, no recorder that reads x between
    the launches of a call; PRCG_XP_DEFER is an option of the handle."""
    from test_distributed import rccl_ids
    L, P = amd['L'], amd['problems']
    A = make_operator(P, 'band')
    n = A.shape[0]
    b, x0, x_true = P.reference_rhs(A, n)
    op = amd['device'].DeviceCSR(A, knobs={'PRCG_SMALL': '0'})
    op.begin(L.PIPE_PR, b, x0, 16, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM)
    assert op.schedule()['fused'] and op.schedule()['xp_deferred'], op.schedule()
    # an option like the others: prcg_set_option takes it per handle (DeviceCSR passes its knobs through it)
    off = amd['device'].DeviceCSR(A, knobs={'PRCG_SMALL': '0', 'PRCG_XP_DEFER': '0'})
    off.begin(L.PIPE_PR, b, x0, 16, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM)
    assert off.schedule()['fused'] and not off.schedule()['xp_deferred'], off.schedule()
    off.close()
    # recorders that read x after every iteration: every launch closes itself
    for bit in (L.HIST_RESIDUAL_2_NORM, L.HIST_ERROR_A_NORM, L.HIST_ERROR_2_NORM):
        op.begin(L.PIPE_PR, b, x0, 16, x_true=x_true, hist_mask=bit)
        assert op.schedule()['fused'] and not op.schedule()['xp_deferred'], (bit, op.schedule())
    # the other solver families have no (x,p) pair array
    op.begin(L.HS, b, x0, 16)
    assert not op.schedule()['xp_deferred']
    op.close()
    # a communicator -- even of one rank -- selects the multi-rank schedules
    uid, path = rccl_ids(1)
    for knobs in ({'PRCG_FUSED_COMM': '0'}, {'PRCG_FUSED_COMM': '1'}):
        comm = amd['device'].DeviceCSR(A, comm_init=(0, 1, uid, path), knobs=knobs)
        comm.begin(L.PIPE_PR, b, x0, 16)
        assert comm.schedule()['comm'] and not comm.schedule()['xp_deferred'], comm.schedule()
        comm.iterate(4)
        comm.sync()
        comm.close()
        uid, path = rccl_ids(1)
