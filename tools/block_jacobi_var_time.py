"""Variable-size point-block Jacobi (prcg_set_block_jacobi_var / prcg_build_block_jacobi_var) against what was there, in one process:
   block_jacobi_var_time.py [part=abc] [workload=s4b_80] [m=80] [repeats=3] [iters=200] [host=1]
     a  `workload` with the UNIFORM partition of size 3: the same blocks through the uniform calls (prcg_build_block_jacobi) and
        through the variable ones -- build time of each (host clock around work that ends in `sync`, legs alternated after a
        warm-up) and a `pipe_pr_pcg` session of `iters` iterations each; the blocks of the two are compared bit for bit
     b  fem_irregular_3d(m) with its nodal partition (problems.fem_irregular_blocks): the device build against the host path
        (VarBlockJacobi: NumPy gather over every nonzero, LAPACK, host re-lay, upload; host=0 skips it), and a `pipe_pr_pcg`
        session of `iters` iterations with the device-built blocks
     c  on the matrix of b: `pipe_pr_pcg` iterations per second with the device-built nodal blocks and with scalar Jacobi
One record per measurement on stderr; ONE JSON line on stdout, with the USEFUL bytes of the apply launches beside each session:
(m + 2) * 8 + 1 per row for the single-vector launch, (m + 4) * 8 + 1 for the pair launch (m: the size of the row's block; the
uniform kernels read no code byte).  The kernels' own times come from a separate run of each part,
   rocprofv3 --kernel-trace --stats -- python tools/block_jacobi_var_time.py part=a repeats=1
(k_block_jacobi_pair<3> against k_block_jacobi_var_pair, k_block_jacobi_build<3> against k_block_jacobi_var_build)."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from new_cg_variants_amd import _lib as L
from new_cg_variants_amd import problems as P
from new_cg_variants_amd.cg_variants import VarBlockJacobi
from new_cg_variants_amd.device import DeviceCSR

opt = dict(part='abc', workload='s4b_80', m='80', repeats='3', iters='200', host='1')
for a in sys.argv[1:]:
    k, _, v = a.partition('=')
    if k not in opt or not v:
        sys.exit(f'unknown argument {a!r}\n{__doc__}')
    opt[k] = v
if set(opt['part']) - set('abc') or not opt['part']:
    sys.exit(__doc__)
repeats, iters = int(opt['repeats']), int(opt['iters'])


def note(**kw):
    print('# ' + json.dumps(kw), file=sys.stderr, flush=True)


def timed(fn, op):
    t = time.perf_counter()
    fn()
    op.sync()
    return (time.perf_counter() - t) * 1e3


def alternate(op, legs):
    """legs: name -> callable; every leg once as a warm-up, then `repeats` times each, alternated: median, min, max in ms"""
    ms = {w: [] for w in legs}
    for rep in range(-1, repeats):
        for w, fn in legs.items():
            dt = timed(fn, op)
            note(leg=w, repeat=rep, ms=dt)
            if rep >= 0:
                ms[w].append(dt)
    return {w: {'median_ms': float(np.median(v)), 'min_ms': min(v), 'max_ms': max(v)} for w, v in ms.items()}


def session(op, b, x0, **kw):
    """a pipe_pr_pcg session of `iters` iterations after 10 of warm-up: us per iteration, the schedule, and whether nu stayed finite"""
    op.begin(L.PIPE_PR, b, x0, iters + 12, **kw)
    op.iterate(10)
    op.sync()
    t = time.perf_counter()
    op.iterate(iters)
    op.sync()
    dt = time.perf_counter() - t
    s = op.schedule()
    return {'us_per_iteration': dt / iters * 1e6, 'iterations_per_second': iters / dt, 'block_jacobi': s['block_jacobi'],
            'block_jacobi_var': s['block_jacobi_var'], 'fused': s['fused'], 'nu_finite': bool(np.isfinite(op.get_scalars(iters + 10)[L.S_NU]))}


def useful_bytes(sizes, code_byte):
    rows = np.repeat(sizes, sizes).astype(np.int64)         # per row the size of its block
    return {'single_launch': int(((rows + 2) * 8 + code_byte).sum()), 'pair_launch': int(((rows + 4) * 8 + code_byte).sum())}


result = {}
if 'a' in opt['part']:
    t0 = time.perf_counter()
    wl = P.WORKLOADS[opt['workload']]
    A = wl['make']().tocsr()
    n, nnz = A.shape[0], int(A.nnz)
    note(workload=wl['desc'], n=n, nnz=nnz, generated_s=time.perf_counter() - t0)
    ptr = np.minimum(np.arange(0, n + 3, 3, dtype=np.int64), n)[:-(-n // 3) + 1]
    op = DeviceCSR(A)
    op.sync()
    legs = alternate(op, {'uniform_build': lambda: op.build_block_jacobi(3), 'var_build': lambda: op.build_block_jacobi_var(ptr)})
    legs['var_build']['ratio_to_uniform'] = legs['var_build']['median_ms'] / legs['uniform_build']['median_ms']
    op.build_block_jacobi(3)
    uni = op.get_block_jacobi()
    op.build_block_jacobi_var(ptr)
    var = op.get_block_jacobi_var()
    m_last = n - 3 * (uni.shape[0] - 1)
    same = np.array_equal(np.concatenate([uni[:-1].reshape(-1), uni[-1, :m_last, :m_last].reshape(-1)]).view(np.uint64), var.view(np.uint64))
    b, x0 = np.random.default_rng(21).standard_normal(n), np.zeros(n)
    sizes = np.diff(ptr)
    result['a'] = {'workload': opt['workload'], 'n': n, 'nnz': nnz, 'build': legs, 'blocks_bit_identical': bool(same),
                   'uniform_session': session(op, b, x0, block_jacobi=(3, None)), 'var_session': session(op, b, x0, block_jacobi_var=(ptr, None)),
                   'useful_bytes_uniform': useful_bytes(sizes, 0), 'useful_bytes_var': useful_bytes(sizes, 1)}
    result['a']['var_session']['ratio_to_uniform'] = result['a']['var_session']['us_per_iteration'] / result['a']['uniform_session']['us_per_iteration']
    op.close()
    del A, op, uni, var

if set('bc') & set(opt['part']):
    t0 = time.perf_counter()
    m = int(opt['m'])
    A = P.fem_irregular_3d(m).tocsr()
    ptr = P.fem_irregular_blocks(m)
    n, nnz = A.shape[0], int(A.nnz)
    assert ptr[-1] == n
    sizes = np.diff(ptr)
    note(workload=f'fem_irregular_3d({m})', n=n, nnz=nnz, blocks=np.bincount(sizes).tolist(), generated_s=time.perf_counter() - t0)
    op = DeviceCSR(A)
    op.sync()
    b, x0 = np.random.default_rng(21).standard_normal(n), np.zeros(n)
    base = {'workload': f'fem_irregular_3d({m})', 'n': n, 'nnz': nnz, 'blocks_of_size': np.bincount(sizes).tolist()}
    if 'b' in opt['part']:
        legs = {'device_build': lambda: op.build_block_jacobi_var(ptr)}
        if opt['host'] == '1':
            legs['host_gather_invert_upload'] = lambda: op.set_block_jacobi_var(ptr, VarBlockJacobi(A, ptr).inv_blocks)
        legs = alternate(op, legs)
        if opt['host'] == '1':
            legs['device_build']['ratio_host_over_this'] = legs['host_gather_invert_upload']['median_ms'] / legs['device_build']['median_ms']
            host = op.get_block_jacobi_var()
            op.build_block_jacobi_var(ptr)
            dev = op.get_block_jacobi_var()
            result_diff = float(np.abs(dev - host).max() / np.abs(host).max())
        else:
            result_diff = None
        result['b'] = dict(base, build=legs, largest_difference_from_lapack_over_largest_entry=result_diff,
                           var_session=session(op, b, x0, block_jacobi_var=(ptr, None)), useful_bytes_var=useful_bytes(sizes, 1))
    if 'c' in opt['part']:
        inv_diag = 1.0 / A.diagonal()
        runs = {'nodal_blocks': [], 'jacobi': []}
        for rep in range(-1, repeats):
            for w, kw in (('nodal_blocks', dict(block_jacobi_var=(ptr, None))), ('jacobi', dict(inv_diag=inv_diag))):
                s = session(op, b, x0, **kw)
                note(leg=w, repeat=rep, **s)
                if rep >= 0:
                    runs[w].append(s)
        result['c'] = dict(base, **{w: {'iterations_per_second_median': float(np.median([s['iterations_per_second'] for s in v])),
                                        'us_per_iteration_median': float(np.median([s['us_per_iteration'] for s in v])),
                                        'fused': v[0]['fused'], 'block_jacobi_var': v[0]['block_jacobi_var']} for w, v in runs.items()})
        result['c']['nodal_over_jacobi_time_per_iteration'] = result['c']['nodal_blocks']['us_per_iteration_median'] / result['c']['jacobi']['us_per_iteration_median']
    op.close()
print(json.dumps(result), flush=True)
