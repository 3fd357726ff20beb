"""tests/rank_group_common.py held to its rules, and the all-pairs walk (tests/handle_walk_common.py) over a group, without a GPU:
the handles are fakes -- plain Python objects with per-rank state whose "sessions" store values into the OTHER ranks' memory (a
shared dict: slot (destination, parity, source) -> (counter, value), counter = (epoch, iteration), as the peer exchange's slots
carry one) and read what the neighbours stored into theirs.  A fake with ONE planted leak of the kind a multi-rank handle could
have -- a ghost parity kept from the session before on one rank, an epoch that an abandoned session does not advance, a refused
begin that leaves a request armed -- must be reported by the walk as exactly the ordered pairs that plant it.  And the condition
on the inputs of tests/test_rank_sessions_after_each_other.py, for all seven groups (the one held back included)."""
import threading

import numpy as np
import pytest
import scipy.sparse as sp

import handle_walk_common as hw
import test_rank_sessions_after_each_other as walk
from rank_group_common import GroupDead, RankGroup, RankTimeout

NRANKS = 3
KINDS = ['even_a', 'odd_a', 'even_b', 'odd_b', 'products', 'refusals']
SESSIONS = KINDS[:4]
ODD = ('odd_a', 'odd_b')
ITERS = {'even_a': 4, 'odd_a': 3, 'even_b': 4, 'odd_b': 3}        # an odd kind ends on the odd parity of the slots
ABANDONED_AT = 2
A = sp.diags([np.full(11, -1.0), np.full(12, 4.0), np.full(11, -1.0)], [-1, 0, 1], format='csr')


class Refused(RuntimeError):
    pass


class Wire:
    """what the ranks share: every rank's slots (the other ranks store into them) and the barrier that stands for the waits"""

    def __init__(self, nranks):
        self.slot = {}
        self.barrier = threading.Barrier(nranks)

    def wait(self):
        self.barrier.wait(timeout=30)


def value(kind, i, src):
    return float(KINDS.index(kind) * 100 + i * 10 + src)


class FakeRank:
    """leak: None, or 'parity' (rank 1 begins on the parity its previous session ended on instead of 0), 'epoch' (a begin right
    after an abandoned session does not advance the epoch, so the new session takes the abandoned one's slots for its own),
    'armed' (a refused begin leaves a request armed; whatever runs next on the rank consumes it).  A product or a refusal ends
    the session that is open."""

    def __init__(self, rank, nranks, wire, leak=None):
        self.rank, self.nranks, self.wire, self.leak = rank, nranks, wire, leak
        self.neighbours = [q for q in (rank - 1, rank + 1) if 0 <= q < nranks]
        self.epoch = self.parity = self.last_end = 0
        self.armed = self.left_open = self.closed = False

    def begin(self, kind):
        self.epoch += 0 if self.leak == 'epoch' and self.left_open else 1
        self.parity = self.last_end if self.leak == 'parity' and self.rank == 1 else 0
        self.stop_at, self.armed = (1 if self.armed else None), False
        self.kind, self.k, self.read = kind, 0, []

    def iterate(self, iters):
        for i in range(self.k, self.k + iters):
            if self.stop_at is not None and i >= self.stop_at:
                break
            par = (self.parity + i) & 1
            self.wire.wait()
            early = {src: self.wire.slot.get((self.rank, par, src)) for src in self.neighbours}
            self.wire.wait()
            for dst in self.neighbours:
                self.wire.slot[(dst, i & 1, self.rank)] = ((self.epoch, i), value(self.kind, i, self.rank))
            self.wire.wait()
            for src in self.neighbours:          # a slot that carried this iteration's counter already is taken without a wait
                e = early[src]
                self.read.append(e[1] if e is not None and e[0] >= (self.epoch, i) else self.wire.slot[(self.rank, par, src)][1])
            self.k = i + 1
            self.last_end = self.k & 1

    def refuse(self):
        was, self.armed = self.armed, self.leak == 'armed'
        raise Refused(f'rank {self.rank}: refused' + (' (a request was armed)' if was else ''))

    def run(self, kind):
        if kind in SESSIONS:
            self.begin(kind)
            self.iterate(ITERS[kind])
            self.left_open = False
            return dict(k=self.k, ghost=np.array(self.read), x=np.full(3, value(kind, self.k, self.rank)))
        self.left_open, self.last_end = False, 0
        if kind == 'products':
            was, self.armed = self.armed, False
            return dict(y=np.full(3, self.rank + (0.5 if was else 0.0)))
        with pytest.raises(Refused) as exc:
            self.refuse()
        return dict(texts=(str(exc.value),))

    def abandon(self, kind):
        if kind in SESSIONS:
            self.begin(kind)
            self.iterate(ABANDONED_AT)
            self.left_open = True

    def close(self):
        self.closed = True


def fake_group(leak=None, nranks=NRANKS, timeout=30, made=None):
    wire = Wire(nranks)

    def factory(r, part, gather_objects):
        op = FakeRank(r, nranks, wire, leak)
        everyone = gather_objects(op)                  # (collective at build, as connect_peer_exchange is)
        assert everyone[r] is op and len(everyone) == nranks
        if made is not None:
            made.extend(everyone if r == 0 else [])
        return op
    return RankGroup(A, nranks, factory=factory, timeout=timeout, gather_timeout=30)


def walked(leak, abandoned):
    """(Walk, fresh) of a fake group with `leak`; fresh: every kind on a group of its own WITHOUT a leak"""
    fresh = {}
    for kind in KINDS:
        g = fake_group()
        fresh[kind] = g.call(lambda op, rank, lo, hi: op.run(kind))
        g.close()
    g = fake_group(leak)
    try:
        got = hw.walk(KINDS, lambda kind: g.call(lambda op, rank, lo, hi: op.run(kind)), fresh,
                      leave=(lambda kind: g.call(lambda op, rank, lo, hi: op.abandon(kind))) if abandoned else None)
    finally:
        g.close()
    assert got.compared == len(KINDS) ** 2 + 1
    return got, fresh


def test_call_runs_the_ranks_at_the_same_time_and_returns_in_rank_order():
    made = []
    g = fake_group(made=made)
    assert [int(x) for x in g.offsets] == [0, 4, 8, 12] and [op.rank for op in made] == [0, 1, 2]
    barrier = threading.Barrier(NRANKS)

    def meet(op, rank, lo, hi):
        barrier.wait(timeout=30)                       # returns only if all ranks are inside fn at the same time
        return threading.current_thread().name, op.rank, lo, hi
    assert g.call(meet) == [('rank-0', 0, 0, 4), ('rank-1', 1, 4, 8), ('rank-2', 2, 8, 12)]
    # rank r returns only after rank r + 1 has: the results arrive in reverse order and come back in rank order
    after = [threading.Event() for _ in range(NRANKS + 1)]
    after[NRANKS].set()
    order = []

    def backwards(op, rank, lo, hi):
        assert after[rank + 1].wait(timeout=30)
        order.append(rank)
        after[rank].set()
        return rank * 10
    assert g.call(backwards) == [0, 10, 20] and order == [2, 1, 0]
    g.close()
    assert all(op.closed for op in made) and not any(t.is_alive() for t in g._threads)
    with pytest.raises(GroupDead):
        g.call(meet)


@pytest.mark.parametrize('abandoned', [False, True])
def test_a_walk_over_a_group_without_a_leak_reports_nothing(abandoned):
    got, fresh = walked(None, abandoned)
    assert got.found == []
    xs = [np.concatenate([r['x'] for r in fresh[kind]]) for kind in SESSIONS]
    assert not any(np.array_equal(a, b) for i, a in enumerate(xs) for b in xs[i + 1:])


def test_a_ghost_parity_kept_on_one_rank_is_found_at_its_pairs_and_names_the_rank():
    got, _ = walked('parity', abandoned=False)
    assert {(a, b) for a, b, _ in got.found} == {(a, b) for a in ODD for b in SESSIONS}, hw.render(KINDS, got.found)
    assert all(paths == ['[1]/ghost'] for _, _, paths in got.found), got.found
    assert "'even_a' after 'odd_b': [1]/ghost" in hw.render(KINDS, got.found)


def test_an_epoch_not_advanced_by_an_abandoned_session_shows_in_the_abandoned_pass_only():
    got, _ = walked('epoch', abandoned=False)
    assert got.found == []
    got, _ = walked('epoch', abandoned=True)
    # the session after an abandoned one takes the abandoned session's slots for its own: another kind's values (its own kind's: the same)
    assert {(a, b) for a, b, _ in got.found} == {(a, b) for a in SESSIONS for b in SESSIONS if a != b}, hw.render(KINDS, got.found)
    assert all(paths == [f'[{r}]/ghost' for r in range(NRANKS)] for _, _, paths in got.found), got.found


@pytest.mark.parametrize('abandoned', [False, True])
def test_a_request_left_armed_by_a_refused_begin_shows_in_every_kind_right_after_the_refusals(abandoned):
    got, _ = walked('armed', abandoned)
    assert {(a, b) for a, b, _ in got.found} == {('refusals', b) for b in KINDS}, hw.render(KINDS, got.found)
    first = {'products': '[0]/y', 'refusals': '[0]/texts[0]'}
    assert all(paths[0] == first.get(b, '[0]/k') for _, b, paths in got.found), got.found


def test_a_rank_that_raises_is_re_raised_and_the_group_is_dead():
    g = fake_group()
    calls = []

    def fn(op, rank, lo, hi):
        calls.append(rank)
        if rank == 1:
            raise ValueError('rank 1 fails')
        return rank
    with pytest.raises(ValueError, match='rank 1 fails') as exc:
        g.call(fn)
    assert exc.value.rank == 1 and exc.value.other_ranks == {} and sorted(calls) == [0, 1, 2]
    assert g.dead is not None and 'rank 1' in g.dead
    with pytest.raises(GroupDead, match='rank 1'):
        g.call(fn)
    assert sorted(calls) == [0, 1, 2]                  # fn was not invoked again
    g.close()
    with pytest.raises(GroupDead):
        g.call(fn)
    assert sorted(calls) == [0, 1, 2]


def test_a_rank_that_never_returns_fails_the_call_within_the_timeout():
    import time
    g = fake_group(timeout=0.2)
    release = threading.Event()
    calls = []

    def fn(op, rank, lo, hi):
        calls.append(rank)
        if rank == 0:
            release.wait(timeout=30)
        return rank
    t0 = time.perf_counter()
    try:
        with pytest.raises(RankTimeout, match=r'ranks \[0\] did not return'):
            g.call(fn)
        assert time.perf_counter() - t0 < 5
        with pytest.raises(GroupDead, match='did not return'):
            g.call(fn)
        assert sorted(calls) == [0, 1, 2]
    finally:
        release.set()
        g.close()


def test_a_handle_that_cannot_be_built_kills_the_group():
    def factory(r, part, gather_objects):
        if r == 2:
            raise OSError('no device')
        return FakeRank(r, NRANKS, None)
    with pytest.raises(OSError, match='no device'):
        RankGroup(A, NRANKS, factory=factory, timeout=30)


@pytest.mark.parametrize('group', list(walk.GROUPS) + list(walk.HELD_BACK))
def test_the_inputs_of_the_rank_walk_keep_every_oracle_run_clear_of_a_breakdown(group):
    """setup()'s assertion, without a GPU: on the group's operator, for every session kind, the oracle in plain summation order
    keeps mu and nu finite and positive and r.r falling from row to row through row 12 -- a comparison bit for bit of runs in
    rounding noise, or of NaNs, would tell little"""
    matrix, nranks, offsets, knobs, peer, flags, family = walk.group_plan(group)
    S = walk.setup(matrix)
    assert 0 < S['rr_end'] < 2e-3 and (S['d'] > 0).all() and np.isfinite(S['b']).all()
    assert (S['x0_warm'] != 0).all()                   # every ghost row of the warm start is nonzero
    assert nranks == {**walk.GROUPS, **walk.HELD_BACK}[group][2] and (offsets is None or len(offsets) == nranks + 1)
    assert len(walk.KINDS) == 15 and list(walk.KINDS)[0] == 'pipe_pr' and len(hw.all_pairs_sequence(len(walk.KINDS))) == 226
