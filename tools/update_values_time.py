"""Time of bringing NEW VALUES on an unchanged pattern to the device, three ways, on one workload in one process:
   update_values_time.py [workload=s4b_80] [legs=abc] [repeats=3] [iters=300] [ceiling=1] [knobs=KEY:V,...]
     a  a fresh DeviceCSR(A_new): host planning and a full upload -- the only way there was before
     b  DeviceCSR.update_values from a host array (prcg_update_values, data_on_device = 0)
     c  DeviceCSR.update_values from a CUDA tensor (data_on_device = 1)
The legs are alternated, `repeats` times each, after one warm-up of every leg; each is timed with the host clock around work
that ends in `sync` (leg a's handle is closed outside the clock).  A_new = D A D with a seeded random positive diagonal; the
updates alternate between A_new and A so that every update changes every value.
iters > 0: microseconds per pipe_pr_cg iteration on the UPDATED handle against a FRESH handle on the same values, `repeats`
windows of `iters` iterations each, alternated -- they run the same arrays, so the figures should agree within their spread.
One record per measurement on stderr; ONE JSON line on stdout: per leg the median, min and max in milliseconds, whether b and c
beat a by more than the spread of the repeats, the iteration figures, the bytes k_sell_set_values must move (8 nnz read + 8 per
padded value written; the padded count is worked out here from the row pointers for slices of 64 consecutive rows, cut slices
not counted) and, with ceiling=1, what prcg_stream_ceiling reaches in this process (mode 1: 2 x 16 B in + 2 x 16 B out per
entry; mode 3: pure streaming read).  The kernel's own time comes from a separate run:
   rocprofv3 --kernel-trace --stats -- python tools/update_values_time.py workload=... legs=c repeats=1 iters=0 ceiling=0"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # first: the library binds to torch's HIP runtime, whose memory leg c's tensor lives in
from new_cg_variants_amd import problems as P, _lib as L
from new_cg_variants_amd.device import DeviceCSR

opt = dict(workload='s4b_80', legs='abc', repeats='3', iters='300', ceiling='1', knobs='')
for a in sys.argv[1:]:
    k, _, v = a.partition('=')
    if k not in opt or (not v and k != 'knobs'):
        sys.exit(f'unknown argument {a!r}\n{__doc__}')
    opt[k] = v
if set(opt['legs']) - set('abc') or not opt['legs']:
    sys.exit(__doc__)
repeats, iters = int(opt['repeats']), int(opt['iters'])
KNOBS = dict(kv.split(':', 1) for kv in opt['knobs'].split(',') if kv) or None

t0 = time.perf_counter()
wl = P.WORKLOADS[opt['workload']]
A = wl['make']().tocsr()
n, nnz = A.shape[0], int(A.nnz)
d = np.random.default_rng(3).uniform(0.5, 1.5, size=n)
A_new = A.copy()
A_new.data = np.repeat(d, np.diff(A.indptr)) * A.data * d[A.indices]
values = [np.ascontiguousarray(A_new.data), np.ascontiguousarray(A.data)]
tensors = [torch.from_numpy(v).to('cuda:0') for v in values] if 'c' in opt['legs'] else None
torch.cuda.synchronize()
print(f'# {wl["desc"]}: n = {n} nnz = {nnz}, generated in {time.perf_counter() - t0:.1f} s', file=sys.stderr, flush=True)
t = time.perf_counter()
op = DeviceCSR(A, knobs=KNOBS)
op.sync()
print(f'# first DeviceCSR(A): {time.perf_counter() - t:.2f} s', file=sys.stderr, flush=True)
sched = op.schedule()
turn = 0


def leg(which):
    """seconds of one leg, and the route an update took"""
    global turn
    if which == 'a':
        t = time.perf_counter()
        fresh = DeviceCSR(A_new, knobs=KNOBS)
        fresh.sync()
        dt = time.perf_counter() - t
        fresh.close()
        return dt, None
    src = (values if which == 'b' else tensors)[turn % 2]
    turn += 1
    t = time.perf_counter()
    route = op.update_values(src)
    op.sync()
    return time.perf_counter() - t, route


result = {'workload': opt['workload'], 'n': n, 'nnz': nnz, 'knobs': KNOBS or {}, 'operator_bytes': op.operator_bytes(), 'repeats': repeats,
          'sliced_rows': sched['sliced_rows'], 'window_codes': sched['window_codes'], 'sorted_windows': sched['sorted_windows'],
          'route': op.values_route()}
ms = {w: [] for w in opt['legs']}
for rep in range(-1, repeats):                    # (-1: the warm-up of every leg)
    for w in opt['legs']:
        dt, route = leg(w)
        print('# ' + json.dumps({'leg': w, 'repeat': rep, 'ms': dt * 1e3, 'route': route}), file=sys.stderr, flush=True)
        if rep >= 0:
            ms[w].append(dt * 1e3)
legs = {w: {'median_ms': float(np.median(v)), 'min_ms': min(v), 'max_ms': max(v)} for w, v in ms.items()}
for w in 'bc':
    if w in legs and 'a' in legs:
        spread = (legs['a']['max_ms'] - legs['a']['min_ms']) + (legs[w]['max_ms'] - legs[w]['min_ms'])
        legs[w]['ratio_a_over_this'] = legs['a']['median_ms'] / legs[w]['median_ms']
        legs[w]['faster_than_a_by_more_than_the_spread'] = bool(legs['a']['median_ms'] - legs[w]['median_ms'] > spread)
result['legs'] = legs

if iters > 0:
    # the updated handle against a fresh one on the same values (the last update left `values[(turn - 1) % 2]`, or A, on the handle)
    now = A if turn == 0 else (A_new if (turn - 1) % 2 == 0 else A)
    fresh = DeviceCSR(now, knobs=KNOBS)
    b = P.reference_rhs(now, n)[0]
    us = {'updated': [], 'fresh': []}
    for rep in range(repeats):
        for name, o in (('updated', op), ('fresh', fresh)):
            o.begin(L.PIPE_PR, b, np.zeros(n), iters + 12)
            o.iterate(8)
            o.sync()
            t = time.perf_counter()
            o.iterate(iters)
            o.sync()
            us[name].append((time.perf_counter() - t) / iters * 1e6)
            print('# ' + json.dumps({'handle': name, 'repeat': rep, 'us_per_iteration': us[name][-1],
                                     'finite': bool(np.isfinite(o.get_scalars(o.k)[L.S_NU]))}), file=sys.stderr, flush=True)
    result['pipe_pr_cg_us_per_iteration'] = {k: {'median': float(np.median(v)), 'min': min(v), 'max': max(v)} for k, v in us.items()}
    fresh.close()

if sched['sliced_rows'] and not sched['sorted_windows']:
    lens = np.diff(A.indptr).astype(np.int64)
    lens = np.concatenate([lens, np.zeros(-n % 64, dtype=np.int64)]).reshape(-1, 64).max(axis=1)
    padded = int((((lens + 1) & ~1) * 64).sum())
    result['relay_bytes'] = {'read': 8 * nnz, 'written': 8 * padded, 'padded_values': padded}
if opt['ceiling'] == '1':
    result['stream_ceiling_gbs'] = {'mode1_in_and_out': op.stream_ceiling(max(n, 1 << 20) * 4, 1), 'mode3_read': op.stream_ceiling(max(n, 1 << 20) * 4, 3)}
op.close()
print(json.dumps(result), flush=True)
