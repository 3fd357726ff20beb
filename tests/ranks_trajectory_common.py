"""TEST INFRASTRUCTURE shared by the whole-trajectory tests of sessions with several ranks (tests/test_trajectory_ranks.py: window
operators; tests/test_trajectory_ranks_irregular.py: sliced rows and CSR-adaptive tiles): one case in the two modes the tests
compare, and the comparison of both with the oracle run under the case's per-rank trees."""
import numpy as np

from device_order import first_mismatch
from ranks_common import run_ranks
from trajectory_common import ALL_METHODS, CHUNKS, FIELD, FOUR, holds_start, run_oracle


def state_vectors(family, jac):
    """the stored vectors a case reads back: x, r, and with Jacobi r~ and, where the family stores it, s~"""
    return ('x', 'r') + ((('rt', 'st') if family in ('pipe', 'pr', 'gv') else ('rt',)) if jac else ())


def chunk_lengths(iters):
    """mode (b): prcg_iterate calls of CHUNKS and the rest"""
    out, k = [], 0
    for c in CHUNKS + (iters,):
        c = min(c, iters - k)
        if c > 0:
            out.append(c)
            k += c
    return out


def first_breakdown(rows):
    """first state at which the oracle's mu or nu is non-positive or not finite; -1: none"""
    v = rows[:, [FIELD['mu'], FIELD['nu']]]
    bad = ~(np.isfinite(v) & (v > 0)).all(axis=1)
    return int(np.argmax(bad)) if bad.any() else -1


def run_mode(L, A, method, nranks, knobs, peer, offsets, inv_diag, iters, recorders, x0=None, product=None):
    """one multi-rank case in mode (a) (recorders: all four, one prcg_iterate call) or (b) (the recurrence residual only, calls of
    CHUNKS and the rest, the state vectors read after each); run_ranks' (offsets, ranks)"""
    variant, family, jac, _ = ALL_METHODS[method]
    return run_ranks(A, nranks, getattr(L, variant), iters, knobs=knobs, inv_diag=inv_diag if jac else None, hist_mask=15 if recorders else 1,
                     offsets=offsets, peer=peer, chunks=None if recorders else chunk_lengths(iters),
                     vectors=() if recorders else state_vectors(family, jac), scalars=True, x0=x0, read_start=x0 is not None and not recorders,
                     product=product)


def hold_ranks_to_oracle(L, label, method, A, b, x_true, jacobi, runs, dots, iters, full, iterations, same_tree, shape_line, x0=None):
    """runs: [mode (a), mode (b)] of run_mode; dots: (dot, dot0) for the oracle, built by the caller from the per-rank trees of
    runs[0]; A: what the device multiplies with (the global matrix, or its LongRowOperator).  The oracle runs `full` iterations
    (with x0: `iters`), its first breakdown state kb is printed with shape_line(ranks), and iters == iterations(kb) is asserted
    (with x0: that there is none).  Then bit for bit in both modes: every inner product the method defines and the coefficients a, b
    of every iteration on rank 0, and every rank's copy of them; one residual history; in (b) the concatenated state vectors at the
    ends of the prcg_iterate calls.  The recorder histories of (a): 1e-13 relative for the three 2-norms, 1e-11 for the A-norm of
    the error (the recorder kernels sum per rank, then the all-reduce)."""
    variant, family, jac, slots = ALL_METHODS[method]
    nranks = len(runs[0][1])
    for a, c in zip(runs[0][1], runs[1][1]):
        assert same_tree(a['layout'], c['layout']) and same_tree(a['start_layout'], c['start_layout'])
    keep = set(runs[1][1][0]['state'])
    vectors = state_vectors(family, jac)
    if x0 is not None:
        keep.remove(0)
        holds_start([np.concatenate([r['state'][0][i] for r in runs[1][1]]) for i in range(len(vectors))], vectors, x0, b, A)
    assert keep == set(np.cumsum(chunk_lengths(iters)).tolist()) and (iters < 41 or keep == {1, 3, 40, iters}), keep
    dot, dot0 = dots
    rows, ref, snaps = run_oracle(method, A, b, x_true, jacobi, (full if x0 is None else iters) + 1, dot, dot0, keep, vectors=vectors, x0=x0)
    kb = first_breakdown(rows)
    print(f'{label}: oracle breakdown at k={kb}; workgroups x waves per rank: {shape_line(runs[0][1])}')
    assert x0 is None or kb < 0, f'the oracle first breaks down at k={kb} under this case\'s trees, within the {iters} iterations of the run'
    assert x0 is not None or iters == iterations(kb), f'the oracle first breaks down at k={kb} under this case\'s trees: the case runs {iterations(kb)} iterations'
    cols = [FIELD[f] for _, f in slots]
    want = rows[:iters + 1, cols]
    assert np.isfinite(want).all() and (want != 0).all()
    want_coef = np.stack([rows[:iters, FIELD['alpha']], rows[1:iters + 1, FIELD['beta']]], axis=1)
    for mode, (_, ranks) in zip('ab', runs):
        got = ranks[0]['scalars'][:, [getattr(L, s) for s, _ in slots]]
        bad = first_mismatch(got, want)
        assert bad < 0, f'({mode}) inner products {[f for _, f in slots]}: first mismatch at k={bad}: got {got[bad]} want {want[bad]}'
        bad = first_mismatch(ranks[0]['coef'], want_coef)
        assert bad < 0, f'({mode}) coefficients: first mismatch at k={bad + 1}: got {ranks[0]["coef"][bad]} want {want_coef[bad]}'
        for q, r in enumerate(ranks[1:], 1):
            assert first_mismatch(r['scalars'][:, [getattr(L, s) for s, _ in slots]], got) < 0, (mode, 'scalars of rank', q)
            assert first_mismatch(r['coef'], ranks[0]['coef']) < 0, (mode, 'coefficients of rank', q)
            assert np.array_equal(r['hist']['updated_residual_2_norm'], ranks[0]['hist']['updated_residual_2_norm']), (mode, 'history of rank', q)
    ha, hb = runs[0][1][0]['hist'], runs[1][1][0]['hist']
    assert np.array_equal(ha['updated_residual_2_norm'], hb['updated_residual_2_norm']) and np.isfinite(hb['updated_residual_2_norm']).all()
    for k in sorted(keep):
        for i, name in enumerate(vectors):
            got = np.concatenate([r['state'][k][i] for r in runs[1][1]])
            differ = int(np.count_nonzero(got != snaps[k][i]))
            assert differ == 0, f'(b) {name} at k={k}: {differ} of {got.size} entries differ, worst {np.max(np.abs(got - snaps[k][i])):.3e}'
    worst = {}
    for q in FOUR:
        want_q = ref[q][:iters + 1]
        assert np.isfinite(want_q).all() and np.isfinite(ha[q]).all() and (want_q > 0).all(), q
        worst[q] = float(np.max(np.abs(ha[q] - want_q) / want_q))
    print(f'   {iters} iterations: inner products, coefficients and {", ".join(vectors)} bit-exact on {nranks} ranks; recorder histories worst rel. deviation ' +
          ', '.join(f'{q} {v:.1e}' for q, v in worst.items()))
    assert worst['updated_residual_2_norm'] <= 1e-13 and worst['residual_2_norm'] <= 1e-13 and worst['error_2_norm'] <= 1e-13, worst
    assert worst['error_A_norm'] <= 1e-11, worst
