"""TEST INFRASTRUCTURE: N > 1 ranks on ONE GPU, the ranks threads of this process connected by tests/transport/libthreads_ccl.so
(a stand-in for librccl.so that moves the collectives' bytes with device-to-device copies; RCCL itself refuses two ranks on one
device).  Real inter-rank data: what rank r reads in its ghost rows was computed by the kernels of rank r +- 1.  Shared by
tests/test_distributed.py (convergence-level assertions) and, through tests/ranks_trajectory_common.py, tests/test_trajectory_ranks.py
and tests/test_trajectory_ranks_irregular.py (whole runs against the oracle)."""
import os
import threading

import numpy as np

from conftest import ROOT


JOIN_TIMEOUT = 240           # seconds a caller waits for a rank thread
GATHER_TIMEOUT = 120         # seconds a rank waits at a barrier of the object all-gather


def transport_path():
    path = os.path.join(ROOT, 'tests', 'transport', 'libthreads_ccl.so')
    assert os.path.exists(path), 'build it with `make` (tests/transport/threads_ccl.hip)'
    return path


def new_unique_id(path):
    """a communicator id of the transport at `path`: one per group of rank handles"""
    from new_cg_variants_amd import _lib as L
    uid = np.zeros(128, dtype=np.uint8)
    L.check(None, L.lib().prcg_comm_unique_id(path.encode(), L.ptr(uid)))
    return uid


def object_gatherer(nranks, timeout=GATHER_TIMEOUT):
    """all-gather of Python objects among the rank threads, which are named 'rank-<r>' (what torch.distributed.all_gather_object is
    between processes)"""
    box = {}
    barrier = threading.Barrier(nranks)
    seq = [0] * nranks

    def gather_objects(obj):
        r = int(threading.current_thread().name.split('-')[-1])
        key = seq[r]
        seq[r] += 1
        box[(key, r)] = obj
        barrier.wait(timeout=timeout)
        res = [box[(key, q)] for q in range(nranks)]
        barrier.wait(timeout=timeout)
        return res
    return gather_objects


def open_rank(r, nranks, part, uid, path, knobs, peer, gather_objects):
    """rank r's handle, on the thread 'rank-<r>': its row block `part` of partition.split_serial with a communicator over the
    transport and its halo plan; knobs: one dict for all ranks or a list, one per rank; peer: the ranks' exchange buffers connected
    (collective: every rank calls this)"""
    from new_cg_variants_amd import partition
    from new_cg_variants_amd.device import DeviceCSR
    A_local, ghost_ids, halo = part
    op = DeviceCSR(A_local, comm_init=(r, nranks, uid.tobytes(), path), halo=halo,
                   knobs=knobs[r] if isinstance(knobs, list) else knobs)
    if peer:
        assert partition.connect_peer_exchange(op, r, gather_objects), 'peer exchange did not connect'
    return op


def run_ranks(A, nranks, variant, iters, knobs=None, inv_diag=None, hist_mask=15, offsets=None, peer=False, chunks=None, x0=None,
              vectors=(), scalars=False, read_start=False, product=None):
    """Solve with `nranks` row blocks, one thread per rank, all on cuda:0: begin(max_iter = iters + 1), then prcg_iterate calls of
    `chunks` (default: one call of `iters`), sync (raises if a wave of a one-launch iteration timed out).
    knobs: one dict for all ranks or a list, one per rank.  peer: connect the ranks' exchange buffers (direct peer exchange; same
    process: device addresses instead of IPC handles).  x0: the GLOBAL start vector (default: problems.reference_rhs's, zeros);
    read_start: the rank's rows of `vectors` are also read right after begin and stored under key 0 of 'state'.
    Returns (offsets, ranks): per rank a dict with 'schedule' (after begin), 'start_layout' and 'layout' (DeviceCSR.layout()
    after begin and after the run), 'hist', 'x', 'y' (the rank's rows of a probe product taken before the session), 'state'
    {k: the rank's rows of the state vectors named in `vectors`, read after each chunk}, and with scalars=True 'scalars'
    (get_scalars(k), k = 0..iters) and 'coef' (get_coefficients(k)[:2], k = 1..iters).  Asserts that the distributed product is
    the global one bit for bit -- SciPy's, or that of product(ranks): the operator as the ranks' kernels multiply it, built from what
    they report (CSR-adaptive tiles sum a long row by a whole wave: device_order.LongRowOperator with the ranks' tile cap)."""
    from new_cg_variants_amd import partition, problems
    path = transport_path()
    n = A.shape[0]
    b, x0_ref, x_true = problems.reference_rhs(A, n)
    x0 = x0_ref if x0 is None else x0
    offsets, parts = partition.split_serial(A, nranks, offsets)
    uid = new_unique_id(path)
    gather_objects = object_gatherer(nranks)
    out = [None] * nranks
    errs = []

    def rank_main(r):
        try:
            lo, hi = int(offsets[r]), int(offsets[r + 1])
            op = open_rank(r, nranks, parts[r], uid, path, knobs, peer, gather_objects)
            y = op.matvec(x_true[lo:hi] * (1.0 + np.arange(lo, hi)))[0]
            op.begin(variant, b[lo:hi], x0[lo:hi], iters + 1, x_true=x_true[lo:hi],
                     inv_diag=None if inv_diag is None else inv_diag[lo:hi], hist_mask=hist_mask)
            res = {'schedule': op.schedule(), 'start_layout': op.layout(), 'state': {}, 'y': y}
            if read_start:
                res['state'][0] = tuple(op.get_vector(v) for v in vectors)
            for c in (chunks or [iters]):
                op.iterate(c)
                if vectors:
                    res['state'][int(op.k)] = tuple(op.get_vector(v) for v in vectors)
            op.sync()
            if scalars:
                res['scalars'] = np.array([op.get_scalars(k) for k in range(iters + 1)])
                res['coef'] = np.array([op.get_coefficients(k)[:2] for k in range(1, iters + 1)])
            res.update(x=op.get_vector('x'), hist=op.history(), layout=op.layout())
            out[r] = res
            op.close()
        except Exception as exc:           # noqa: BLE001 -- reported by the caller
            errs.append((r, repr(exc)))

    threads = [threading.Thread(target=rank_main, args=(r,), name=f'rank-{r}', daemon=True) for r in range(nranks)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=JOIN_TIMEOUT)         # (daemon threads: a rank that never returns fails the test instead of hanging pytest)
    assert not errs, errs
    assert all(o is not None for o in out), 'a rank did not finish'
    y = np.concatenate([o['y'] for o in out])
    assert np.array_equal(y, (A if product is None else product(out)) @ (x_true * (1.0 + np.arange(n)))), 'distributed SpMV differs from the global product'
    return np.asarray(offsets, dtype=np.int64), out


def run_ranks_in_threads(A, nranks, variant, iters, knobs=None, inv_diag=None, hist_mask=15, offsets=None, peer=False, chunks=None):
    """run_ranks as tests/test_distributed.py takes it: (x, histories of rank 0, schedules)."""
    _, out = run_ranks(A, nranks, variant, iters, knobs=knobs, inv_diag=inv_diag, hist_mask=hist_mask, offsets=offsets, peer=peer, chunks=chunks)
    return np.concatenate([o['x'] for o in out]), out[0]['hist'], [o['schedule'] for o in out]
