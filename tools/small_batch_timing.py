"""Shared by tools/small_batch_time.py, small_batch_jacobi_time.py and small_batch_stop_time.py: the systems, the command line,
one timed session and the summary of its windows.  Method: a leg is timed with the host clock around work that ends in a
synchronise; two figures per window, `solve` = begin + iterations (what a caller waits for) and `iterate` = the iterations alone;
the best and the median of the windows are reported."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import scipy.sparse as sp
from new_cg_variants_amd import problems

# the nine test systems of tests/small_batch_common.py
NINE = ['bcsstk03', 'nos4', 'bcsstm22', 'nos7', 'lap32x32', '494_bus', 'model_48_8_3', 'lap40x40', 'lap33x32']


def load_system(name):
    """(A, b): a tests/golden fixture with its right-hand side, or lapNXxNY = laplace_2d(NX, NY) with b = ones"""
    if name.startswith('lap'):
        nx, ny = (int(q) for q in name[3:].split('x'))
        A = problems.laplace_2d(nx, ny)
        return A, np.ones(A.shape[0])
    z = np.load(os.path.join(ROOT, 'tests', 'golden', f'matrix_{name}.npz'))
    n = int(z['n'])
    return sp.csr_matrix((z['data'], z['indices'], z['indptr']), shape=(n, n)), np.asarray(z['b'], dtype=np.float64)


def options(defaults, doc):
    """key=value arguments over `defaults` (strings); anything else ends the run with the tool's docstring"""
    opt = dict(defaults)
    for a in sys.argv[1:]:
        k, _, v = a.partition('=')
        if k not in opt or not v:
            sys.exit(f'unknown argument {a!r}\n{doc}')
        opt[k] = v
    return opt


def timed(session, variant, b, x0, iters, **begin):
    """one window of a DeviceBatch or DeviceCSR session: (solve, iterate) in seconds"""
    t0 = time.perf_counter()
    session.begin(variant, b, x0, iters + 1, hist_mask=1, **begin)
    t1 = time.perf_counter()
    session.iterate(iters)
    session.sync()
    t2 = time.perf_counter()
    return t2 - t0, t2 - t1


def timed_loop(op, variant, B, X0, iters, **begin):
    """the systems one after another on one DeviceCSR: the sums of their windows"""
    return tuple(np.sum([timed(op, variant, b, x0, iters, **begin) for b, x0 in zip(B, X0)], axis=0))


def summary(samples):
    a = np.array(samples) * 1e3
    return {'solve_ms_best': float(a[:, 0].min()), 'solve_ms_median': float(np.median(a[:, 0])),
            'iterate_ms_best': float(a[:, 1].min()), 'iterate_ms_median': float(np.median(a[:, 1]))}
