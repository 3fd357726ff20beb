"""TEST INFRASTRUCTURE: a group of rank handles that LIVES ACROSS CALLS.  tests/ranks_common.run_ranks starts rank threads that do one
fixed thing -- build a handle, run one session, close; this group keeps `nranks` threads alive, each the owner of one handle built
exactly as run_ranks builds its own (ranks_common.open_rank: a DeviceCSR on the rank's row block with a communicator over
tests/transport/libthreads_ccl.so, its halo plan and, with peer=True, the connected peer exchange), and runs whatever a caller hands
it on all of them at the same time, as often as the caller likes: session after session on the same handles
(tests/test_rank_sessions_after_each_other.py).  Not collected; tests/test_rank_group.py holds it to its rules with fake handles,
without a GPU.

  group = RankGroup(A, nranks, knobs=..., offsets=..., peer=...)
  group.call(fn)      fn(op, rank, lo, hi) on every rank at the same time; the results in rank order
  group.close()       closes the handles and ends the threads

An exception on any rank is re-raised by `call` in the caller, after every rank has returned or the join timeout has passed (the
lowest rank's, with `.rank` set and the others' in `.other_ranks`); a rank that does not return within the timeout is an error of
its own (RankTimeout).  After either the group is DEAD: every later call raises GroupDead at once and runs nothing -- after an error
of the device nothing more is to run on it (handle_walk_common.walk) -- and close() only ends the threads that can be ended.  The
threads are daemons: a stuck rank fails the test instead of hanging pytest."""
import queue
import threading

import numpy as np

from ranks_common import GATHER_TIMEOUT, JOIN_TIMEOUT, new_unique_id, object_gatherer, open_rank, transport_path


class RankTimeout(RuntimeError):
    """a rank did not return from a call within the timeout"""


class GroupDead(RuntimeError):
    """the group has had a rank raise or time out, or is closed: nothing more runs on it"""


def real_handles(nranks, knobs=None, peer=False):
    """the handle factory of a real group: factory(r, part, gather_objects) -> ranks_common.open_rank's handle, one communicator id
    for the group"""
    path = transport_path()
    uid = new_unique_id(path)
    return lambda r, part, gather_objects: open_rank(r, nranks, part, uid, path, knobs, peer, gather_objects)


class RankGroup:
    def __init__(self, A, nranks, knobs=None, offsets=None, peer=False, factory=None, timeout=JOIN_TIMEOUT, gather_timeout=GATHER_TIMEOUT):
        """A: the GLOBAL matrix, cut into `nranks` row blocks at `offsets` (None: even) by partition.split_serial.  factory(r, part,
        gather_objects) -> the handle of rank r, called on the thread 'rank-<r>' (default: real_handles(nranks, knobs, peer));
        timeout: seconds `call` waits for a rank; gather_timeout: seconds a rank waits for the others in gather_objects"""
        from new_cg_variants_amd import partition
        self.nranks, self.timeout = int(nranks), timeout
        offsets, self.parts = partition.split_serial(A, nranks, offsets)
        self.offsets = np.asarray(offsets, dtype=np.int64)
        self._factory = real_handles(nranks, knobs, peer) if factory is None else factory
        self._gather = object_gatherer(nranks, timeout=gather_timeout)
        self._ops = [None] * nranks
        self._todo = [queue.Queue() for _ in range(nranks)]
        self.dead = None                       # why nothing more runs: None while the group lives
        self._threads = [threading.Thread(target=self._rank_main, args=(r,), name=f'rank-{r}', daemon=True) for r in range(nranks)]
        for t in self._threads:
            t.start()
        try:
            self._on_all(self._open)
        except BaseException:
            for q in self._todo:                   # (no group: the threads that can still be ended are)
                q.put(None)
            raise

    def _open(self, r):
        self._ops[r] = self._factory(r, self.parts[r], self._gather)

    def _rank_main(self, r):
        while True:
            job = self._todo[r].get()
            if job is None:
                return
            work, done = job
            try:
                done.put((r, True, work(r)))
            except BaseException as exc:           # noqa: BLE001 -- re-raised by the caller
                done.put((r, False, exc))

    def _on_all(self, work):
        """work(r) on every rank thread at the same time; the results in rank order, or the group dies"""
        if self.dead is not None:
            raise GroupDead(f'the group runs nothing more: {self.dead}')
        done = queue.Queue()
        for q in self._todo:
            q.put((work, done))
        out, errs = {}, {}
        for _ in range(self.nranks):
            try:
                r, ok, value = done.get(timeout=self.timeout)
            except queue.Empty:
                break
            (out if ok else errs)[r] = value
        late = [r for r in range(self.nranks) if r not in out and r not in errs]
        if errs:
            r = min(errs)
            self.dead = f'rank {r} raised {errs[r]!r}' + (f'; ranks {late} did not return' if late else '')
            exc = errs[r]
            exc.rank, exc.other_ranks = r, {q: e for q, e in errs.items() if q != r}
            raise exc
        if late:
            self.dead = f'ranks {late} did not return within {self.timeout} s'
            raise RankTimeout(self.dead)
        return [out[r] for r in range(self.nranks)]

    def call(self, fn):
        """fn(op, rank, lo, hi) on every rank at the same time (op: the rank's handle, [lo, hi): its rows of the global system);
        returns the per-rank results in rank order"""
        return self._on_all(lambda r: fn(self._ops[r], r, int(self.offsets[r]), int(self.offsets[r + 1])))

    def close(self):
        """close the handles (a living group only: nothing more runs on a dead one) and end the threads"""
        alive = self.dead is None
        try:
            if alive:
                self._on_all(lambda r: self._ops[r].close())
        finally:
            if self.dead is None:
                self.dead = 'closed'
            for q in self._todo:
                q.put(None)
            if alive and self.dead == 'closed':          # (a dead group's threads may be stuck: daemons, not waited for)
                for t in self._threads:
                    t.join(timeout=self.timeout)
