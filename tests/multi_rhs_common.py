"""TEST INFRASTRUCTURE of the multi-RHS session tests (tests/test_multi_rhs.py, _pr.py, _pipe.py, 4.py, _block_jacobi.py and
tests/multi_block_common.py): ONE copy of what they all need.  Not collected.

  amd                 the package fixture; a test file imports it by name
  same / assert_column_bits / assert_finite      equal bits (NaN equals NaN), no tolerance anywhere
  two_rhs / four_rhs / operator / KNOBS / problem / reference       the cases; oracle runs are computed once and shared, read-only
  oracle_column       one column of the oracle.  It chooses NOTHING: the method, its keyword arguments (dot=, preconditioner=,
                      square=, dot0=), the sum that gives the recorded r.r and the vectors the column reports are the caller's,
                      because each of them decides the bits a session is held to.  hs_column / pr_column: the calls that the
                      Hestenes-Stiefel / predict-and-recompute file and the four-RHS file both make
  device_columns      a session on the device -- `begin` opens it, so every entry is served -- iterated in chunks and read
                      through the per-column getters
  single_session / _raises
"""
import functools

import numpy as np
import pytest

import oracle.ne_oracle as orc
from device_order import device_dot

VECS = ('x', 'r', 'p', 's')
KEYS = VECS + ('rt', 'st', 'scalars', 'alpha', 'beta', 'nu_pred', 'hist')
HS_KEYS = VECS + ('rt', 'scalars', 'alpha', 'beta', 'hist')       # what a Hestenes-Stiefel column is compared in


@pytest.fixture(scope='module')
def amd():
    import new_cg_variants_amd.cg_variants as cgv
    import new_cg_variants_amd.callbacks as cbs
    from new_cg_variants_amd import _lib, device, problems
    return dict(cgv=cgv, cbs=cbs, L=_lib, device=device, problems=problems)


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def dot(a, b):                       # numpy scalars: 0 / 0 is NaN as on the device, not Python's ZeroDivisionError
    return np.float64(device_dot(a, b))


def oracle_column(method, A, b, x0, iters, vecs=VECS, tilde=(), scalars=(0, 1, 2, 3, 4), rr=None, **how):
    """`method` of the oracle (orc.hs_cg, orc.pr_pcg, ...) called with exactly the keyword arguments `how`: the state after `iters`
    iterations (`vecs`, and of rt / st those named in `tilde`: the others are None), the sums [mu, delta, gamma, nu, rr][scalars]
    of every iteration (delta, gamma and the predicted nu of a Hestenes-Stiefel state stay 0), the coefficients used BY every
    iteration >= 1 and the history the device records.  rr(st): the recorded r.r, by default in device_dot's order."""
    rows = []
    rr = rr or (lambda st: dot(st.r, st.r))

    def tap(st):
        rows.append((st.mu, st.dl, st.gm, st.nu, rr(st), st.alpha, st.beta, st.nu_pred))
    with np.errstate(all='ignore'):
        st = method(A, b, x0, iters + 1, tap=tap, **how)['_final_state']
        rows = np.array(rows, dtype=np.float64)
        res = {v: getattr(st, v) for v in vecs}
        res.update({v: getattr(st, v) if v in tilde else None for v in ('rt', 'st')})
        res.update(scalars=rows[:, list(scalars)],
                   alpha=rows[:-1, 5],          # a used BY iteration k = nu / mu of iteration k - 1
                   beta=rows[1:, 6], nu_pred=rows[1:, 7], hist=np.sqrt(rows[:, 4]))
    for v in res.values():
        if v is not None:
            v.setflags(write=False)
    return res


def hs_column(A, b, x0, iters, jacobi, rt_without_jacobi):
    """hs_cg -- called without a preconditioner -- or hs_pcg with orc.jacobi(A), neither with square=: the scalars are mu, nu, rr.
    rt_without_jacobi: report the oracle's rt in that case too (tests/test_multi_rhs.py does; tests/test_multi_rhs4.py reports None)."""
    how = dict(preconditioner=orc.jacobi(A)) if jacobi else {}
    return oracle_column(orc.hs_pcg if jacobi else orc.hs_cg, A, b, x0, iters, tilde=('rt',) if jacobi or rt_without_jacobi else (),
                         scalars=(0, 3, 4), dot=dot, **how)


def pr_column(A, b, x0, iters, jacobi, variant='pr'):
    """pr_pcg / m_pcg with orc.jacobi(A) or the identity `lambda v: v`, and the device's a * a; rt, st only with Jacobi"""
    return oracle_column({'pr': orc.pr_pcg, 'm': orc.m_pcg}[variant], A, b, x0, iters, tilde=('rt', 'st') if jacobi else (),
                         preconditioner=orc.jacobi(A) if jacobi else (lambda v: v), dot=dot, square=lambda a: a * a)


def device_columns(op, L, begin, iters, nrhs, vecs, served, chunks=(1, 2, 7), report=None):
    """The session `begin()` opens on `op` (with iters + 1 as its max_iter and the updated-residual history), read through the
    per-column getters: per column `vecs` (rt, st: None where not among them), ALL scalar slots of every iteration and the slots
    `report` (default: `served`, outside which every slot must be 0), the three coefficients of every iteration >= 1 and the
    history; and the schedule."""
    begin()
    sched = op.schedule()
    for c in chunks:                                    # calls of any length give the same session
        op.iterate(min(c, iters - op.k))
    op.iterate(iters - op.k)
    op.sync()
    assert op.k == iters
    cols = []
    for j in range(nrhs):
        sc = np.array([op.get_scalars(k, rhs=j) for k in range(iters + 1)])
        other = [q for q in range(L.NUM_SCALARS) if q not in served]
        assert not sc[:, other].any(), 'slots the session does not serve are 0'
        cf = np.array([op.get_coefficients(k, rhs=j) for k in range(1, iters + 1)]).reshape(iters, 3)
        col = dict(rt=None, st=None)
        col.update({v: op.get_vector(v, rhs=j) for v in vecs})
        col.update(all_scalars=sc, scalars=sc[:, list(report or served)], alpha=cf[:, 0], beta=cf[:, 1], nu_pred=cf[:, 2],
                   hist=op.history(rhs=j)['updated_residual_2_norm'])
        cols.append(col)
    return cols, sched


def served_slots(L, hs):
    """the scalar slots a session fills: mu, nu, rr; predict-and-recompute and pipelined sessions delta and gamma too"""
    return (L.S_MU, L.S_NU, L.S_RR) if hs else (L.S_MU, L.S_DELTA, L.S_GAMMA, L.S_NU, L.S_RR)


def assert_column_bits(got, want, what, keys=KEYS):
    for q in keys:
        if want[q] is None:
            assert got[q] is None, (what, q)
            continue
        g, w = np.asarray(got[q]), np.asarray(want[q])
        assert g.shape == w.shape, (what, q, g.shape, w.shape)
        if not same(g, w):
            bad = np.argwhere(~((g == w) | (np.isnan(g) & np.isnan(w))))
            raise AssertionError(f'{what}: {q} differs in {len(bad)} of {g.size} entries, first at {bad[0]}: '
                                 f'got {g[tuple(bad[0])]!r} want {w[tuple(bad[0])]!r}')


def assert_finite(want, what):
    """a case whose oracle run breaks down is a wrong case: it fails, it is not skipped (scalars: mu, delta, gamma, nu, rr)"""
    assert np.isfinite(want['scalars']).all() and np.isfinite(want['x']).all(), f'{what}: the oracle run must stay finite'
    assert (want['scalars'][:, [0, 3]] > 0).all(), f'{what}: mu, nu > 0 in the oracle run'


def two_rhs(P, A, seed=7):
    n = A.shape[0]
    b0 = P.reference_rhs(A, n)[0]
    b1 = np.random.default_rng(seed).standard_normal(n)
    return np.stack([b0, b1])


def four_rhs(A):
    """reference_rhs(A, n)[0] and default_rng(s).standard_normal(n) for s = 7, 8, 9: columns 0 and 1 are those of two_rhs"""
    from new_cg_variants_amd import problems as P
    n = A.shape[0]
    return np.stack([P.reference_rhs(A, n)[0]] + [np.random.default_rng(s).standard_normal(n) for s in (7, 8, 9)])


def _workload(name):
    from new_cg_variants_amd import problems as P
    return P.WORKLOADS[name]['make']()


def _problems(fn, *args):
    from new_cg_variants_amd import problems as P
    return getattr(P, fn)(*args)


def _golden(name):
    from conftest import load_matrix
    return load_matrix(name)[0]


# One operator per product family of the multi-vector products: name -> (how to make it, the `family` keys every session on it
# reports through schedule()).  What only one session type reports (the pipelined session's spmm4) that file overlays; a file
# with operators of its own adds them here.
OPERATORS = {
    # banded, 15 diagonals: window tiles with index streams
    's3_small': (functools.partial(_workload, 's3_small'), dict(window=True, pattern=False, sliced_rows=False)),
    # 5-point stencil, 64 x 48
    's1_small': (functools.partial(_workload, 's1_small'), dict(window=True, pattern=True, sliced_rows=False)),
    # 7-point stencil, odd extents: pattern tiles, several workgroups, a ragged last tile
    'lap3d': (functools.partial(_problems, 'laplace_3d', 21, 17, 13), dict(window=True, pattern=True, sliced_rows=False)),
    # n = 1,050,804 > 2048 * 512: two trips per block of the vector kernels, a ragged last block
    'lap3d_two_trips': (functools.partial(_problems, 'laplace_3d', 102, 102, 101), dict(window=True)),
    # 3 unknowns per node, 27-point coupling: sliced rows
    'fem12': (functools.partial(_problems, 'fem_like_3d', 12), dict(window=False, sliced_rows=True, sorted_windows=False)),
    # 1 / 3 / 6 unknowns per node, thinned coupling: sliced rows of varying length
    'fem_irregular10': (functools.partial(_problems, 'fem_irregular_3d', 10), dict(window=False, sliced_rows=True)),
    # golden matrix, what the planner picks for it: sliced rows
    'bcsstk14': (functools.partial(_golden, 'bcsstk14'), dict(window=False, sliced_rows=True)),
    # ... and with the sliced layout switched off (KNOBS): the CSR-adaptive tiles
    'bcsstk14_csr': (functools.partial(_golden, 'bcsstk14'), dict(window=False, sliced_rows=False)),
}
KNOBS = {'bcsstk14_csr': {'PRCG_SELL': '0'}}


@functools.lru_cache(maxsize=None)
def operator(name):
    """(A, family) of OPERATORS; `family` is asserted through schedule()."""
    make, family = OPERATORS[name]
    return make(), dict(family)


@functools.lru_cache(maxsize=None)
def problem(name, nrhs, x0_nonzero=False):
    """(A, B, X0) of an operator, read-only: the right-hand sides of two_rhs / four_rhs"""
    from new_cg_variants_amd import problems as P
    A, _ = operator(name)
    n = A.shape[0]
    B = two_rhs(P, A) if nrhs == 2 else four_rhs(A)
    X0 = np.random.default_rng(11).standard_normal((nrhs, n)) if x0_nonzero else np.zeros((nrhs, n))
    B.setflags(write=False)
    X0.setflags(write=False)
    return A, B, X0


@functools.lru_cache(maxsize=None)
def reference(oracle, nrhs, name, variant, jacobi, iters, x0_nonzero, column):
    """oracle(A, b, x0, iters, jacobi, variant) -- a test file's own oracle_column -- of one column of problem(name, nrhs,
    x0_nonzero), computed once and shared (read-only).  column: 0 .. nrhs - 1, or 'zero' (b = 0, x0 = 0)."""
    A, B, X0 = problem(name, nrhs, x0_nonzero)
    if column == 'zero':
        return oracle(A, np.zeros(A.shape[0]), np.zeros(A.shape[0]), iters, jacobi, variant)
    return oracle(A, B[column], X0[column], iters, jacobi, variant)


def single_session(op, L, variant, b, x0, iters, inv_diag=None, vecs=VECS):
    op.begin(variant, b, x0, iters + 1, inv_diag=inv_diag, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM)
    sched = op.schedule()
    op.iterate(iters)
    op.sync()
    vec = {v: op.get_vector(v) for v in vecs}
    sc = np.array([op.get_scalars(k) for k in range(iters + 1)])
    cf = np.array([op.get_coefficients(k) for k in range(1, iters + 1)])
    return sched, vec, sc, cf, op.history()['updated_residual_2_norm']


def _raises(L, text):
    return pytest.raises(L.PrcgError, match=text)
