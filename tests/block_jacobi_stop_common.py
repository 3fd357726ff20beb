"""TEST INFRASTRUCTURE of tests/test_block_jacobi_stop.py: the table of cases, the systems and block-Jacobi objects they name, the
oracle's free-running trajectory of a pipelined session with a block preconditioner under the device's summation order, and one
device session read back in full.  The stopping rule, stop_of and holds_trajectory are tests/single_stop_common.py's.

In a block-Jacobi session (the stored-tilde schedule) all five sums of every row -- mu, delta, gamma, nu and r.r, row 0 included
-- are taken by the pipelined update kernel and closed by the 256-thread final tree: device_order.device_dot, which depends on n
alone."""
import numpy as np

from device_order import device_dot
from single_stop_common import BREAKDOWN, CONVERGED, rule

VECTORS = ('x', 'r', 'p', 's', 'w', 'u', 'rt', 'st', 'ut', 'wt')
CHUNKS = (1, 2, 37)                    # prcg_iterate calls without a sync between them, then the rest
# variant -> the oracle's flavour
FLAVOUR = {'PIPE_PR': 'pr', 'PIPE_PR_M': 'pr_m', 'PIPE_P': 'p', 'PIPE_P_M': 'p_m'}
# system -> (matrix, knobs of the handle besides PRCG_SMALL=0, operator family the handle must report)
SYSTEMS = {
    'fem16': ('fem16', {}, 'sliced'),                        # fem_like_3d(16, 3), n = 12 288: 192 full slices
    'fem16_csr': ('fem16', {'PRCG_SELL': '0'}, 'csr'),       # ... as CSR-adaptive tiles
    'irr20': ('irr20', {}, 'sliced'),                        # fem_irregular_3d(20), n = 24 025: a ragged last slice
    'nos7': ('nos7', {}, 'window'),                          # golden, n = 729 = 182 * 4 + 1: six window tiles, a short last block
    'bcsstk03': ('bcsstk03', {}, 'window'),                  # golden, n = 112 = 14 * 8: one window tile
    'lap2d_300': ('lap2d_300', {}, 'window'),                # laplace_2d(300, 200), n = 60 000 = 8571 * 7 + 3: 938 tiles
}
# blocks -> (kind, argument): 'bj' BlockJacobi(A, bs) from the host, 'bj_built' built on the device (DeviceBlockJacobi), 'bjv' /
# 'bjv_built' the same with a partition ('nodal': problems.fem_irregular_blocks(20); 'cyc8': sizes 1..8 cyclic)
BLOCKS = {'bs3': ('bj', 3), 'bs4': ('bj', 4), 'bs7': ('bj', 7), 'bs8': ('bj', 8), 'built3': ('bj_built', 3),
          'nodal': ('bjv', 'nodal'), 'built_nodal': ('bjv_built', 'nodal'), 'cyc8': ('bjv', 'cyc8')}
# (system, blocks, variant, rtol, max_iter, how the oracle must stop)
CASES = [
    ('fem16', 'bs3', 'PIPE_PR', 1e-8, 80, CONVERGED),
    ('fem16_csr', 'built3', 'PIPE_P', 1e-6, 80, None),       # (None: converged or broken down, as the blocks read back decide)
    ('irr20', 'nodal', 'PIPE_PR_M', 1e-6, 100, CONVERGED),
    ('irr20', 'built_nodal', 'PIPE_PR', 1e-6, 100, None),
    ('nos7', 'bs4', 'PIPE_PR', 1e-8, 140, CONVERGED),
    ('nos7', 'bs4', 'PIPE_PR_M', 1e-10, 140, BREAKDOWN),
    ('nos7', 'bs4', 'PIPE_P_M', 1e-8, 140, BREAKDOWN),
    ('bcsstk03', 'bs8', 'PIPE_P_M', 1e-13, 120, BREAKDOWN),
    ('bcsstk03', 'cyc8', 'PIPE_PR', 1e-8, 230, CONVERGED),
    ('lap2d_300', 'bs7', 'PIPE_PR', 1e-2, 150, CONVERGED),
]


def case_id(c):
    return '-'.join(str(q) for q in c[:5])


def cyclic_partition(n):
    """block sizes 1, 2, .. 8, 1, 2, .. (the last one cut to fit): tests/test_trajectory_stored_tilde.py's"""
    sizes = []
    while sum(sizes) < n:
        sizes.append(min(len(sizes) % 8 + 1, n - sum(sizes)))
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


_systems, _blocks, _trajectories = {}, {}, {}


def system(matrices, name):
    """matrix name -> (A, b), built once per process and left unchanged"""
    from new_cg_variants_amd import problems as P
    if name not in _systems:
        make = {'lap2d_300': lambda: P.laplace_2d(300, 200), 'fem16': lambda: P.fem_like_3d(16, 3), 'irr20': lambda: P.fem_irregular_3d(20)}
        if name in make:
            A = make[name]().tocsr()
            b = P.reference_rhs(A, A.shape[0])[0]
        else:
            A, z = matrices[name]
            b = np.asarray(z['b'], dtype=np.float64)
        _systems[name] = (A, b)
    return _systems[name]


def block_object(matrices, matrix, blocks):
    """the host object of (matrix, blocks), built once per process: BlockJacobi / VarBlockJacobi (LAPACK inverses, handed to the
    device) or DeviceBlockJacobi / DeviceVarBlockJacobi (the host restatement of the device build)"""
    import new_cg_variants_amd.cg_variants as cgv
    from new_cg_variants_amd import problems as P
    if (matrix, blocks) not in _blocks:
        A = system(matrices, matrix)[0]
        kind, arg = BLOCKS[blocks]
        ptr = None if not kind.startswith('bjv') else P.fem_irregular_blocks(20) if arg == 'nodal' else cyclic_partition(A.shape[0])
        _blocks[(matrix, blocks)] = {'bj': lambda: cgv.BlockJacobi(A, arg), 'bj_built': lambda: cgv.DeviceBlockJacobi(A, arg),
                                     'bjv': lambda: cgv.VarBlockJacobi(A, ptr), 'bjv_built': lambda: cgv.DeviceVarBlockJacobi(A, ptr)}[kind]()
    return _blocks[(matrix, blocks)]


def begin_keyword(blocks, M):
    """the keyword of DeviceCSR.begin for these blocks"""
    kind, arg = BLOCKS[blocks]
    return {'bj': lambda: {'block_jacobi': (arg, M.inv_blocks)}, 'bj_built': lambda: {'block_jacobi': (arg, None)},
            'bjv': lambda: {'block_jacobi_var': (M.block_ptr, M.inv_blocks)}, 'bjv_built': lambda: {'block_jacobi_var': (M.block_ptr, None)}}[kind]()


def with_blocks_read_back(A, blocks, M, read):
    """the object whose __call__ applies the blocks the device built (`read`, asserted equal to the restatement's)"""
    import new_cg_variants_amd.cg_variants as cgv
    kind, arg = BLOCKS[blocks]
    assert read.shape == M.inv_blocks.shape and np.array_equal(read, M.inv_blocks), int(np.count_nonzero(read != M.inv_blocks))
    N = cgv.DeviceBlockJacobi(A, arg) if kind == 'bj_built' else cgv.DeviceVarBlockJacobi(A, M.block_ptr)
    if kind == 'bjv_built':
        N._layout()
    N._inv_blocks = np.ascontiguousarray(read)
    return N


def threshold(b, rtol):
    import new_cg_variants_amd.cg_variants as cgv
    return float(cgv._stop_thresholds('threshold', rtol, None, [b])[0])


def _dot(a, b):                 # (not a Python float: nu / mu must give inf / nan at a breakdown, not raise)
    return np.float64(device_dot(a, b))


def trajectory(A, b, variant, M, iters, thr=None, x0=None, key=None):
    """The oracle (oracle/ne_oracle.py: pipe_start / pipe_advance with prec=M) from x0 (None: zeros), every inner product and r.r
    by device_dot: row k of `scalars` = {mu, delta, gamma, nu, rr} of state k, row k - 1 of `coef` = {a, b, predicted nu} of
    iteration k.  It runs `iters` iterations, or, with a threshold, up to and including the first state the rule fires at (the rows
    behind a stop are not part of a stopped run and nothing reads them); `at[k]`: the ten vectors of the LAST state k it reached.
    A breakdown leaves inf / nan behind, as the reference does.  key: cache the result under it (and leave it unchanged)."""
    import oracle.ne_oracle as O
    if key is not None and key in _trajectories:
        return _trajectories[key]
    with np.errstate(all='ignore'):
        st = O.pipe_start(A, b, np.zeros(b.size) if x0 is None else x0, prec=M, dot=_dot)
        scalars, coef = [[st.mu, st.dl, st.gm, st.nu, _dot(st.r, st.r)]], []
        while st.k < iters and not (thr is not None and rule(scalars[-1][0], scalars[-1][3], scalars[-1][4], thr)):
            a = st.alpha
            O.pipe_advance(A, st, flavour=FLAVOUR[variant], prec=M, dot=_dot, square=lambda q: q * q)
            coef.append([a, st.beta, st.nu_pred])
            scalars.append([st.mu, st.dl, st.gm, st.nu, _dot(st.r, st.r)])
    out = dict(scalars=np.array(scalars, dtype=np.float64), coef=np.array(coef, dtype=np.float64).reshape(-1, 3),
               at={st.k: {v: np.array(getattr(st, v), copy=True) for v in VECTORS}})
    if key is not None:
        _trajectories[key] = out
    return out


def read_session(op, max_iter):
    return dict(k=int(op.k), stop=op.stop(), at={v: op.get_vector(v) for v in VECTORS},
                scalars=np.array([op.get_scalars(k) for k in range(max_iter)]),
                coef=np.array([op.get_coefficients(k) for k in range(1, max_iter)]).reshape(-1, 3),
                hist=op.history()['updated_residual_2_norm'])


def run_session(L, op, variant, b, max_iter, rr_stop, chunks, begin_kw, then=0, x0=None):
    """one device session with the recurrence residual recorded: prcg_iterate calls of `chunks` (each cut to what is left) WITHOUT a
    synchronisation between them, then the rest, then ONE prcg_sync; everything the session holds is read back.  then > 0: a
    further prcg_iterate(then) and a second reading (`again`)."""
    op.begin(getattr(L, variant), b, np.zeros(b.size) if x0 is None else x0, max_iter, hist_mask=1, rr_stop=rr_stop, **begin_kw)
    out = {'schedule': op.schedule()}
    left = max_iter - 1
    for c in tuple(chunks) + (max_iter,):
        c = min(c, left)
        op.iterate(c)
        left -= c
    op.sync()
    out.update(read_session(op, max_iter))
    if then:
        op.iterate(then)
        op.sync()
        out['again'] = read_session(op, max_iter)
    return out
