"""The walk of tests/test_every_session_after_every_other.py one level up, where the contract really is "any function after any
other on the same A": cg_variants caches ONE DeviceCSR per matrix so that every solver function runs on it.  25 calls that between
them use every begin path and every preconditioner object are made through the cached operator so that every ordered pair of
calls, self-pairs included, is consecutive exactly once (tests/handle_walk_common.py: 626 calls), and every call is compared, on
the 64-bit patterns of every array of every trial dict it returns (NaNs included) plus 'iterations' / 'status' where present,
with the same call made right after clear_operator_cache(): a freshly uploaded operator is the reference.  The walk must never
upload A a second time: len(_OPERATORS) stays 1 and the cached object is the same one throughout.

Two matrices: s3_small (window tiles, value dictionary, n = 20 000) and fem_like_3d(12) (sliced rows); the systems, right-hand
sides, block objects and thresholds are those of tests/test_every_session_after_every_other.setup.  max_iter = 13.  Every single
call takes all four recorder callbacks and x_true; the multi-RHS functions serve the recurrence residual alone and take that.

Thresholds: the two stopping calls whose session is one of that module's stopping kinds take its threshold as rtol = sqrt(thr) /
||b|| (hs_pcg_stop with Jacobi: hs_thr; pipe_pr_pcg without a preconditioner: pipe_thr -- both lie between two oracle rows with a
margin of 1e-3, which the rounding of sqrt and the square does not use up) and must stop converged at that module's plan on the
fresh operator; the block-Jacobi and two-RHS calls take rtol from bj_thr / rhs_thr the same way and stop wherever that puts them.

Measured on an MI355X (every pair equal on both matrices, one upload per walk): s3_small 1.9 s, fem12 1.6 s."""
import numpy as np
import pytest

import handle_walk_common as hw
from test_every_session_after_every_other import setup

MAX_ITER = 13
MATRICES = ('s3_small', 'fem12')


def calls(name):
    """label -> a function of no arguments that makes the call and returns its trial dict(s); built once per matrix"""
    import new_cg_variants_amd.callbacks as cbs
    import new_cg_variants_amd.cg_variants as cgv
    S = setup(name)
    A, b, n = S['A'], S['b'], S['n']
    x0, X2, X4 = np.zeros(n), np.zeros((2, n)), np.zeros((4, n))
    four = [cbs.error_A_norm, cbs.residual_2_norm, cbs.error_2_norm, cbs.updated_residual_2_norm]
    x_true = np.random.default_rng(7).standard_normal(n)            # b = A @ this vector (setup's b)
    assert np.array_equal(A @ x_true, b)
    kw = dict(callbacks=four, x_true=x_true)
    mkw = dict(callbacks=[cbs.updated_residual_2_norm])
    import scipy.sparse as sp
    shifted = sp.csr_matrix(A + 0.5 * sp.diags(A.diagonal()))
    jac = cgv.Jacobi(A)
    host3, hostv = cgv.BlockJacobi(shifted, 3), cgv.VarBlockJacobi(shifted, S['ptr'])
    built3, builtv = cgv.DeviceBlockJacobi(A, 3), cgv.DeviceVarBlockJacobi(A, S['ptr'])
    w = np.sqrt(S['inv_diag'])

    def neighbours(v):               # symmetric positive definite and no diagonal scaling: applied on the host
        q = w * v
        return w * (q + 0.01 * (np.roll(q, 1) + np.roll(q, -1)))
    norm = float(np.linalg.norm(b))

    def rtol(thr, of=norm):
        return float(np.sqrt(thr)) / of
    norms2 = [float(np.linalg.norm(S['B2'][c])) for c in range(2)]

    def single(fn, *prec, **more):
        return lambda: getattr(cgv, fn)(A, b, x0, MAX_ITER, *prec, **kw, **more)

    def multi(fn, B, X0, *prec, **more):
        return lambda: getattr(cgv, fn)(A, B, X0, MAX_ITER, *prec, **mkw, **more)

    def same_values_again():
        same_values_again.routes.append(cgv.update_values(A))        # (None right after clear_operator_cache: nothing to update)
        return cgv.pipe_pr_cg(A, b, x0, MAX_ITER, **kw)
    same_values_again.routes = []
    return {
        'hs_cg': single('hs_cg'), 'cg_cg': single('cg_cg'), 'gv_cg': single('gv_cg'), 'pr_cg': single('pr_cg'), 'pipe_pr_cg': single('pipe_pr_cg'),
        'hs_pcg jacobi': single('hs_pcg', jac), 'cg_pcg jacobi': single('cg_pcg', jac), 'gv_pcg jacobi': single('gv_pcg', jac),
        'm_pcg jacobi': single('m_pcg', jac), 'pipe_p_m_pcg jacobi': single('pipe_p_m_pcg', jac),
        'gv_pcg w_replace': single('gv_pcg', jac, w_replace=lambda k, **_: k % 3 == 0),
        'pipe_pr_pcg callable': single('pipe_pr_pcg', neighbours),
        'pipe_pr_pcg rtol': single('pipe_pr_pcg', None, rtol=rtol(S['pipe_thr'])),
        'hs_pcg_stop rtol': single('hs_pcg_stop', jac, rtol=rtol(S['hs_thr'])),
        'pipe_pr_bpcg built3 rtol': single('pipe_pr_bpcg', built3, rtol=rtol(S['bj_thr'])),
        'pipe_p_bpcg host3': single('pipe_p_bpcg', host3),
        'pr_pcg built var': single('pr_pcg', builtv),
        'hs_pcg host var': single('hs_pcg', hostv),
        'hs_cg_multi 2': multi('hs_cg_multi', S['B2'], X2),
        'pr_pcg_multi 4': multi('pr_pcg_multi', S['B4'], X4, jac),
        'pipe_pr_pcg_multi rtol': multi('pipe_pr_pcg_multi', S['B2'], X2, jac, rtol=[rtol(S['rhs_thr'][c], norms2[c]) for c in range(2)]),
        'pipe_pr_m_cg_multi': multi('pipe_pr_m_cg_multi', S['B2'], X2),
        'hs_bpcg_multi 4 built3': multi('hs_bpcg_multi', S['B4'], X4, built3),
        'pr_bpcg_multi host var': multi('pr_bpcg_multi', S['B2'], X2, hostv),
        'update_values, pipe_pr_cg': same_values_again,
    }


def reading(out):
    """what a call returned, floating-point arrays as their bit patterns"""
    if isinstance(out, dict):
        return {key: reading(v) for key, v in out.items()}
    if isinstance(out, (list, tuple)):
        return [reading(v) for v in out]
    if isinstance(out, np.ndarray) and out.dtype == np.float64:
        return np.ascontiguousarray(out).view(np.uint64)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('name', MATRICES)
def test_every_call_after_every_other_equals_a_freshly_uploaded_operator(name):
    import time
    import new_cg_variants_amd.cg_variants as cgv
    S = setup(name)
    table = calls(name)
    kinds = list(table)
    K = len(kinds)
    t0 = time.perf_counter()
    fresh = {}
    try:
        for kind in kinds:
            cgv.clear_operator_cache()
            fresh[kind] = reading(table[kind]())
        for kind, plan in (('pipe_pr_pcg rtol', S['pipe_stop']), ('hs_pcg_stop rtol', S['hs_stop'])):
            assert (fresh[kind]['iterations'], fresh[kind]['status']) == (plan[0], 'converged'), (name, kind, fresh[kind]['iterations'], fresh[kind]['status'], plan)
        for kind in kinds:
            trials = fresh[kind] if isinstance(fresh[kind], list) else [fresh[kind]]
            assert all('updated_residual_2_norm' in t and t['updated_residual_2_norm'].shape == (MAX_ITER,) for t in trials), (name, kind)
        t1 = time.perf_counter()
        cgv.clear_operator_cache()
        seen = []
        routes = table['update_values, pipe_pr_cg'].routes
        del routes[:]

        def run(kind):
            out = reading(table[kind]())
            assert len(cgv._OPERATORS) == 1, (name, kind, 'the walk uploaded A a second time')
            seen.append(next(iter(cgv._OPERATORS.values())))
            assert seen[-1] is seen[0], (name, kind, 'the cached operator was replaced')
            return out
        got = hw.walk(kinds, run, fresh)
        want = 'replanned' if name == 's3_small' else 'in_place'
        assert routes == [want] * K, (name, 'update_values found and updated the cached operator every time', routes)
    finally:
        cgv.clear_operator_cache()
    print(f'{name}: {got.compared} calls compared, {len(got.found)} differ; fresh operators {t1 - t0:.2f} s, walk {time.perf_counter() - t1:.2f} s')
    assert K == 25 and got.compared == K * K + 1 == 626 and len(set(zip(got.sequence, got.sequence[1:]))) == K * K
    assert not got.found, f'{name}:\n' + hw.render(kinds, got.found)
