"""TEST INFRASTRUCTURE of the all-pairs walks (tests/test_every_session_after_every_other.py, and whatever walks another object
later): a sequence of K * K + 1 runs in which every ordered pair of K kinds, self-pairs included, is consecutive exactly once; the
walker that runs it on ONE object and compares every run with the same kind's run on an object that has never run anything else;
and the K x K picture of what differed.  Not collected; tests/test_handle_walk.py holds it to planted leaks without a GPU.

The sequence is an Euler circuit of the complete digraph with loops on K vertices -- every vertex has K edges in and K out, so
one exists -- found by Hierholzer's algorithm: walk unused edges until stuck (which can only happen at the start vertex), then
splice in the detours of vertices that still have unused edges; the stack does the splicing."""
import collections

import numpy as np

Walk = collections.namedtuple('Walk', 'found compared sequence')
Walk.__doc__ = """found: [(predecessor, kind, paths)] of every run that differed from the fresh one (predecessor None: the very first run);
compared: how many runs were compared; sequence: the kinds in the order they ran"""


def all_pairs_sequence(K):
    """K * K + 1 indices in 0 .. K - 1, beginning and ending with 0: every ordered pair (a, b), a == b included, occurs exactly
    once as (seq[i], seq[i + 1])"""
    assert K >= 1
    unused = [0] * K                     # vertex v has used its edges to 0 .. unused[v] - 1
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if unused[v] < K:
            stack.append(unused[v])
            unused[v] += 1
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


def segments(sequence, parts):
    """the sequence cut into `parts` consecutive pieces that overlap by ONE run, so that every consecutive pair of the sequence is a
    consecutive pair of exactly one piece: for a walk too long for one test, each piece on a walked object of its own"""
    edges = len(sequence) - 1
    assert 1 <= parts <= max(edges, 1)
    cuts = [edges * i // parts for i in range(parts + 1)]
    return [sequence[lo:hi + 1] for lo, hi in zip(cuts, cuts[1:])]


def differences(a, b, path=''):
    """the paths at which two readings differ (np.array_equal at the leaves): tests/test_stop_kinds_share_a_handle.py's"""
    if isinstance(a, dict):
        return [f'{path}: keys'] if not isinstance(b, dict) or a.keys() != b.keys() else \
            [d for key in a for d in differences(a[key], b[key], f'{path}/{key}')]
    if isinstance(a, (list, tuple)) and not np.isscalar(a):
        return [f'{path}: length'] if not isinstance(b, (list, tuple)) or len(a) != len(b) else \
            [d for i, (x, y) in enumerate(zip(a, b)) for d in differences(x, y, f'{path}[{i}]')]
    if a is None or b is None:
        return [] if a is b else [path]
    return [] if np.array_equal(np.asarray(a), np.asarray(b)) else [path]


def walk(kinds, run, fresh, leave=None, sequence=None, catch=()):
    """Run all_pairs_sequence(len(kinds)) -- or `sequence`, a piece of it (segments) -- on ONE object: run(kind) runs a kind on the
    walked object and returns its reading, fresh[kind] (or fresh(kind)) is the reading of the same kind on an object that has run
    nothing else: the reference.  leave(kind), if given, is called after every compared run but the last, before the next kind
    begins: what a caller does to leave the object in a worse state than a finished run does.  EVERY differing run is collected,
    none stops the walk.  catch: exception types that count as a difference of the run that raised them, at the path 'raised: ...'
    (a refusal); anything else ends the walk -- after an error of the device nothing more is to run on it."""
    sequence = all_pairs_sequence(len(kinds)) if sequence is None else list(sequence)
    want = fresh if callable(fresh) else fresh.__getitem__
    found, before = [], None
    for i, q in enumerate(sequence):
        kind = kinds[q]
        try:
            paths = differences(run(kind), want(kind))
        except catch as exc:
            paths = [f'raised: {type(exc).__name__}: {exc}']
        if paths:
            found.append((before, kind, paths))
        if leave is not None and i + 1 < len(sequence):
            leave(kind)
        before = kind
    return Walk(found, len(sequence), [kinds[q] for q in sequence])


def render(kinds, found, paths=4):
    """the K x K matrix of failing pairs -- row: the predecessor, column: the kind that differed, so what A leaves behind shows as
    a row and what leaks into B as a column -- and under it every failing pair with its first `paths` paths"""
    kinds = list(kinds)
    bad = {(a, b) for a, b, _ in found}
    width = len(str(len(kinds) - 1))
    lines = [f'{len(bad)} of {len(kinds) ** 2} ordered pairs differ from the fresh object (row: predecessor, column: kind)',
             ' ' * (width + 1) + ' '.join(f'{j:>{width}}' for j in range(len(kinds)))]
    for i, a in enumerate(kinds):
        lines.append(f'{i:>{width}} ' + ' '.join(f'{"X" if (a, b) in bad else ".":>{width}}' for b in kinds) + f'   {a}')
    for a, b, where in found:
        more = f' (+{len(where) - paths} more)' if len(where) > paths else ''
        lines.append(f'{b!r} after {a!r}: {", ".join(where[:paths])}{more}')
    return '\n'.join(lines)
