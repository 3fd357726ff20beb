"""TEST INFRASTRUCTURE of tests/test_multi_rhs_stop.py: the columns of a pipelined two-RHS session stopped at their own thresholds
(prcg.h: prcg_set_stop_rhs).  Not collected.

  stop_of             the rule (small_batch_common.rule) walked over the oracle's rows: the FIRST row at which it fires
  case                thresholds taken from the oracle alone -- rr of column 0's row i, of column 1's row j -- and where the
                      oracle then stops each column
  frozen              what a column stopped at k holds: the oracle's state of iteration k (the run of the shared reference
                      truncated to k + 1 rows, rerun for k iterations for the vectors), every later row and entry zero
  session / read      a session with thresholds on the device, iterated by the calls the test names, read through the
                      per-column getters in the style of multi_rhs_common.device_columns

The operators, the right-hand sides (two_rhs, x0 = 0) and the reference columns are those of tests/test_multi_rhs_pipe.py:
one oracle run per (operator, flavour, preconditioner, column, iterations), computed once and shared, read-only.
"""
import numpy as np

import multi_rhs_common as common
import test_multi_rhs_pipe as pipe
from multi_rhs_common import same
from small_batch_common import rule

ITERS = 60                       # the iterations of the shared reference runs: rows 0 .. 60, a session of max_iter 61
KEYS = pipe.KEYS
ALL = KEYS + ('all_scalars',)


def stop_of(rows, thr):
    """(k, status) of the first row [mu delta gamma nu rr] at which the rule fires under the threshold thr, else (-1, 0)"""
    for k, row in enumerate(np.asarray(rows)):
        verdict = rule(row[0], row[3], row[4], thr)
        if verdict:
            return k, verdict
    return -1, 0


def reference(matrix, flavour, jacobi, column, iters=ITERS):
    return pipe.reference(matrix, flavour, jacobi, iters, False, column)


def case(matrix, flavour, jacobi, i, j, iters=ITERS):
    """thresholds (rr of column 0's oracle row i, of column 1's row j; None: 0.0) and the oracle's (k, status) per column"""
    rows = [reference(matrix, flavour, jacobi, c, iters)['scalars'] for c in range(2)]
    thr = [0.0 if q is None else float(rows[c][q, 4]) for c, q in enumerate((i, j))]
    return thr, [stop_of(rows[c], thr[c]) for c in range(2)]


def frozen(matrix, flavour, jacobi, column, k, iters=ITERS):
    """Column `column` stopped at k: the vectors of the oracle's iteration k (its run for k iterations), rows 0 .. k of the shared
    run's scalars, coefficients 1 .. k and history entries 0 .. k, zero beyond"""
    full = reference(matrix, flavour, jacobi, column, iters)
    at = reference(matrix, flavour, jacobi, column, k)
    assert same(at['scalars'], full['scalars'][:k + 1]) and same(at['hist'], full['hist'][:k + 1]), 'the truncated run IS the run for k iterations'
    res = {v: at[v] for v in pipe.VECS + ('rt', 'st')}
    scalars = np.zeros((iters + 1, 5))
    scalars[:k + 1] = full['scalars'][:k + 1]
    hist = np.zeros(iters + 1)
    hist[:k + 1] = full['hist'][:k + 1]
    res.update(scalars=scalars, hist=hist)
    for q in ('alpha', 'beta', 'nu_pred'):
        v = np.zeros(iters)
        v[:k] = full[q][:k]
        res[q] = v
    return res


def read(op, L, iters, jacobi):
    """per column what multi_rhs_common.device_columns reads, from the session as it stands (synchronised); with the stops and k"""
    served = common.served_slots(L, False)
    other = [q for q in range(L.NUM_SCALARS) if q not in served]
    cols = []
    for j in range(2):
        sc = np.array([op.get_scalars(k, rhs=j) for k in range(iters + 1)])
        assert not sc[:, other].any(), 'slots the session does not serve are 0'
        cf = np.array([op.get_coefficients(k, rhs=j) for k in range(1, iters + 1)]).reshape(iters, 3)
        col = dict(rt=None, st=None)
        col.update({v: op.get_vector(v, rhs=j) for v in pipe.VECS + (('rt', 'st') if jacobi else ())})
        col.update(all_scalars=sc, scalars=sc[:, list(served)], alpha=cf[:, 0], beta=cf[:, 1], nu_pred=cf[:, 2],
                   hist=op.history(rhs=j)['updated_residual_2_norm'])
        cols.append(col)
    return cols, op.stops_rhs(), op.k


def session(op, L, variant, B, X0, iters, inv_diag, rr_stop, calls, after=None):
    """A session with the thresholds rr_stop; `calls`: the lengths of its prcg_iterate calls, each followed by prcg_sync --
    after(i) is then called with the session open.  Returns read()."""
    op.begin_multi_pipe(variant, B, X0, iters + 1, inv_diag=inv_diag, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM, rr_stop=rr_stop)
    for i, c in enumerate(calls):
        op.iterate(c)
        op.sync()
        if after is not None:
            after(i)
    return read(op, L, iters, inv_diag is not None)


def assert_equal_columns(got, want, what, keys=ALL):
    common.assert_column_bits(got, want, what, keys=keys)
