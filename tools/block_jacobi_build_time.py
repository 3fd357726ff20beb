"""Time of getting the block-Jacobi inverses of the operator ON the handle, two ways, bs = 3, on one workload in one process:
   block_jacobi_build_time.py [workload=s4b_80] [legs=ab] [repeats=3] [bs=3] [ceiling=1] [bytes=1]
     a  BlockJacobi(A, bs) on the host (NumPy gather over every nonzero, LAPACK) plus prcg_set_block_jacobi (host re-lay and
        upload) -- the only way there was before
     b  prcg_build_block_jacobi: one kernel pass over the operator already resident
The legs are alternated, `repeats` times each, after one warm-up of every leg; each is timed with the host clock around work
that ends in `sync`.  One record per measurement on stderr; ONE JSON line on stdout: per leg the median, min and max in
milliseconds, whether b beats a by more than the summed spread of the two legs' repeats, the largest difference of the device
inverses from LAPACK's relative to the block's largest entry, with bytes=1 the bytes the kernel must move (4 B per nonzero of
columns, 4 B per row pointer, the 64-byte value lines that hold a matching entry, the block store) and, with ceiling=1, what
prcg_stream_ceiling reaches in this process (mode 3: pure streaming read).  The kernel's own time comes from a separate run:
   rocprofv3 --kernel-trace --stats -- python tools/block_jacobi_build_time.py workload=... legs=b repeats=1 ceiling=0 bytes=0"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from new_cg_variants_amd import problems as P
from new_cg_variants_amd.cg_variants import BlockJacobi
from new_cg_variants_amd.device import DeviceCSR

opt = dict(workload='s4b_80', legs='ab', repeats='3', bs='3', ceiling='1', bytes='1')
for a in sys.argv[1:]:
    k, _, v = a.partition('=')
    if k not in opt or not v:
        sys.exit(f'unknown argument {a!r}\n{__doc__}')
    opt[k] = v
if set(opt['legs']) - set('ab') or not opt['legs']:
    sys.exit(__doc__)
repeats, bs = int(opt['repeats']), int(opt['bs'])

t0 = time.perf_counter()
wl = P.WORKLOADS[opt['workload']]
A = wl['make']().tocsr()
n, nnz = A.shape[0], int(A.nnz)
print(f'# {wl["desc"]}: n = {n} nnz = {nnz}, generated in {time.perf_counter() - t0:.1f} s', file=sys.stderr, flush=True)
t = time.perf_counter()
op = DeviceCSR(A)
op.sync()
print(f'# DeviceCSR(A): {time.perf_counter() - t:.2f} s', file=sys.stderr, flush=True)
sched = op.schedule()
host_blocks = None


def leg(which):
    """seconds of one leg"""
    global host_blocks
    t = time.perf_counter()
    if which == 'a':
        prec = BlockJacobi(A, bs)
        op.set_block_jacobi(bs, prec.inv_blocks)
        op.sync()
        dt = time.perf_counter() - t
        host_blocks = prec.inv_blocks
        return dt
    op.build_block_jacobi(bs)
    op.sync()
    return time.perf_counter() - t


result = {'workload': opt['workload'], 'n': n, 'nnz': nnz, 'bs': bs, 'repeats': repeats, 'sliced_rows': sched['sliced_rows'],
          'operator_bytes': op.operator_bytes()}
ms = {w: [] for w in opt['legs']}
for rep in range(-1, repeats):                    # (-1: the warm-up of every leg)
    for w in opt['legs']:
        dt = leg(w)
        print('# ' + json.dumps({'leg': w, 'repeat': rep, 'ms': dt * 1e3}), file=sys.stderr, flush=True)
        if rep >= 0:
            ms[w].append(dt * 1e3)
legs = {w: {'median_ms': float(np.median(v)), 'min_ms': min(v), 'max_ms': max(v)} for w, v in ms.items()}
if 'a' in legs and 'b' in legs:
    spread = (legs['a']['max_ms'] - legs['a']['min_ms']) + (legs['b']['max_ms'] - legs['b']['min_ms'])
    legs['b']['ratio_a_over_this'] = legs['a']['median_ms'] / legs['b']['median_ms']
    legs['b']['summed_spread_ms'] = spread
    legs['b']['faster_than_a_by_more_than_the_spread'] = bool(legs['a']['median_ms'] - legs['b']['median_ms'] > spread)
result['legs'] = legs

if 'b' in opt['legs'] and host_blocks is not None:
    op.build_block_jacobi(bs)
    dev = op.get_block_jacobi()
    err = np.abs(dev - host_blocks).max(axis=(1, 2)) / np.abs(host_blocks).max(axis=(1, 2))
    result['largest_difference_from_lapack'] = float(err.max())

if opt['bytes'] == '1':
    tr = 256 - 256 % bs
    touched, r0, last_line = 0, 0, -1
    while r0 < n:                                  # value lines that hold a matching entry, in chunks of rows
        r1 = min(n, r0 + (1 << 20))
        lo, hi = int(A.indptr[r0]), int(A.indptr[r1])
        rows = np.repeat(np.arange(r0, r1), np.diff(A.indptr[r0:r1 + 1]))
        q = np.flatnonzero((A.indices[lo:hi] // bs) == (rows // bs)) + lo
        lines = np.unique(q // 8)
        touched += int(lines.size) - (1 if r0 > 0 and lines.size and lines[0] == last_line else 0)
        if lines.size:
            last_line = int(lines[-1])
        r0 = r1
    store = -(-n // tr) * bs * 256 * 8
    result['kernel_bytes'] = {'columns': 4 * nnz, 'row_pointers': 4 * (n + 1), 'value_lines_touched': 64 * touched, 'block_store': store,
                              'total': 4 * nnz + 4 * (n + 1) + 64 * touched + store}
if opt['ceiling'] == '1':
    result['stream_ceiling_gbs'] = {'mode3_read': op.stream_ceiling(max(n, 1 << 20) * 4, 3)}
op.close()
print(json.dumps(result), flush=True)
