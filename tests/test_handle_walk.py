"""tests/handle_walk_common.py held to what it promises, without a GPU: the sequence covers every ordered pair exactly once, and a
walk over a stub object with ONE planted leak reports exactly that pair -- an ordinary one, a self-pair, the pair of the circuit's
last edge, and one that shows only after the `leave` step."""
import collections

import numpy as np
import pytest

import handle_walk_common as hw

KINDS = [f'kind{i}' for i in range(7)]


@pytest.mark.parametrize('K', [1, 2, 5, 23])
def test_every_ordered_pair_occurs_exactly_once(K):
    seq = hw.all_pairs_sequence(K)
    assert len(seq) == K * K + 1 and set(seq) == set(range(K))
    pairs = collections.Counter(zip(seq, seq[1:]))
    assert len(pairs) == K * K and set(pairs.values()) == {1}, [p for p, c in pairs.items() if c != 1]


@pytest.mark.parametrize('K,parts', [(5, 1), (5, 3), (23, 4), (2, 4)])
def test_segments_lose_no_pair(K, parts):
    """pieces that overlap by one run: the pairs of the pieces together are the pairs of the sequence, each once"""
    seq = hw.all_pairs_sequence(K)
    pieces = hw.segments(seq, parts)
    assert len(pieces) == parts and pieces[0][0] == seq[0] and pieces[-1][-1] == seq[-1]
    assert all(a[-1] == b[0] for a, b in zip(pieces, pieces[1:]))
    pairs = collections.Counter(p for piece in pieces for p in zip(piece, piece[1:]))
    assert pairs == collections.Counter(zip(seq, seq[1:]))


class Stub:
    """an object whose run of `into` reads one value that a run of `after` (abandoned=False) or an abandoned run of `after`
    (abandoned=True) left behind; every other run depends on its kind alone"""

    def __init__(self, after=None, into=None, abandoned=False):
        self.after, self.into, self.abandoned = after, into, abandoned
        self.stale = False

    def run(self, kind):
        leaked = self.stale and kind == self.into
        self.stale = kind == self.after and not self.abandoned
        q = float(KINDS.index(kind))
        return dict(k=12, stop=(-1, 0), cols=[dict(x=np.full(5, q), r=None), dict(x=np.full(5, q + (0.5 if leaked else 0)), r=None)],
                    scalars=np.arange(6.0).reshape(2, 3) + q)

    def leave(self, kind):
        if self.abandoned:
            self.stale = kind == self.after


FRESH = {kind: Stub().run(kind) for kind in KINDS}
SEQ = [KINDS[q] for q in hw.all_pairs_sequence(len(KINDS))]


def test_a_walk_without_a_leak_reports_nothing():
    stub = Stub()
    got = hw.walk(KINDS, stub.run, FRESH, leave=stub.leave)
    assert got.found == [] and got.compared == len(KINDS) ** 2 + 1 and got.sequence == SEQ


@pytest.mark.parametrize('after,into', [('kind2', 'kind5'), ('kind3', 'kind3'), (SEQ[-2], SEQ[-1]), (SEQ[0], SEQ[1])],
                         ids=['ordinary', 'self', 'last edge', 'first edge'])
def test_a_planted_leak_is_reported_as_exactly_its_pair(after, into):
    stub = Stub(after, into)
    got = hw.walk(KINDS, stub.run, FRESH)
    assert got.found == [(after, into, ['/cols[1]/x'])], got.found
    assert got.compared == len(KINDS) ** 2 + 1
    picture = hw.render(KINDS, got.found)
    rows = picture.splitlines()[2:2 + len(KINDS)]
    marks = [(i, j) for i, row in enumerate(rows) for j, c in enumerate(row.split()[1:1 + len(KINDS)]) if c == 'X']
    assert marks == [(KINDS.index(after), KINDS.index(into))], picture
    assert f'{into!r} after {after!r}: /cols[1]/x' in picture


def test_a_leak_that_needs_the_leave_step():
    """left behind by an ABANDONED run only: a walk without the step sees nothing, the walk with it exactly the pair"""
    stub = Stub('kind4', 'kind1', abandoned=True)
    assert hw.walk(KINDS, stub.run, FRESH).found == []
    stub = Stub('kind4', 'kind1', abandoned=True)
    assert hw.walk(KINDS, stub.run, FRESH, leave=stub.leave).found == [('kind4', 'kind1', ['/cols[1]/x'])]


def test_every_difference_is_collected_and_a_raising_run_is_one():
    """two planted pairs and a kind that raises after one predecessor: all of them, in walk order, none stops the walk"""
    a, b = Stub('kind0', 'kind6'), Stub('kind6', 'kind2')

    def run(kind):
        ra, rb = a.run(kind), b.run(kind)
        if kind == 'kind5' and run.before == 'kind1':
            run.before = kind
            raise RuntimeError('refused')
        run.before = kind
        return ra if hw.differences(ra, FRESH[kind]) else rb
    run.before = None
    got = hw.walk(KINDS, run, FRESH, catch=(RuntimeError,))
    assert sorted((p, k) for p, k, _ in got.found) == [('kind0', 'kind6'), ('kind1', 'kind5'), ('kind6', 'kind2')]
    assert [w for p, k, w in got.found if k == 'kind5'] == [['raised: RuntimeError: refused']]
    assert got.compared == len(KINDS) ** 2 + 1
    run.before = None
    with pytest.raises(RuntimeError, match='refused'):            # not asked to catch it: the walk ends there
        hw.walk(KINDS, run, FRESH)


def test_segments_of_a_walk_report_the_same_pair():
    found, compared = [], 0
    for piece in hw.segments(hw.all_pairs_sequence(len(KINDS)), 3):
        stub = Stub('kind2', 'kind5')
        got = hw.walk(KINDS, stub.run, FRESH, sequence=piece)
        found += got.found
        compared += got.compared
    assert found == [('kind2', 'kind5', ['/cols[1]/x'])] and compared == len(KINDS) ** 2 + 3


def test_differences_names_the_paths():
    a = dict(k=3, at=dict(x=np.arange(3.0), r=None), cols=[(1, 0), (2, 1)])
    assert hw.differences(a, dict(k=3, at=dict(x=np.arange(3.0), r=None), cols=[(1, 0), (2, 1)])) == []
    assert hw.differences(a, dict(k=4, at=dict(x=np.arange(3.0), r=np.zeros(3)), cols=[(1, 0), (2, 2)])) == ['/k', '/at/r', '/cols[1][1]']
    assert hw.differences(a, dict(k=3, at=dict(x=np.arange(3.0)), cols=[(1, 0)])) == ['/at: keys', '/cols: length']
