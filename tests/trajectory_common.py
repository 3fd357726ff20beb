"""TEST INFRASTRUCTURE shared by the whole-trajectory tests (tests/test_trajectory_oracle.py: window operators;
tests/test_trajectory_irregular.py: sliced rows and CSR-adaptive tiles; tests/test_trajectory_stored_tilde.py: block-Jacobi and
host-callback sessions on either): the method table, one oracle run with taps and one device session in either of the two
modes the tests compare."""
import numpy as np

from oracle import ne_oracle as orc

FOUR = ['error_A_norm', 'residual_2_norm', 'error_2_norm', 'updated_residual_2_norm']

# method -> (device variant, family, Jacobi, [(device scalar slot, oracle state field)]: the inner products the method defines)
PIPE_SLOTS = [('S_MU', 'mu'), ('S_DELTA', 'dl'), ('S_GAMMA', 'gm'), ('S_NU', 'nu')]
LAG_SLOTS = [('S_MU', 'mu'), ('S_DELTA', 'eta'), ('S_NU', 'nu')]        # (mu is derived: eta - (b / a) nu, cg_cg.py:67)
HS_SLOTS = [('S_MU', 'mu'), ('S_NU', 'nu')]
METHODS = {
    'pipe_pr_pcg': ('PIPE_PR', 'pipe', True, PIPE_SLOTS), 'pipe_p_pcg': ('PIPE_P', 'pipe', True, PIPE_SLOTS),
    'pipe_pr_m_pcg': ('PIPE_PR_M', 'pipe', True, PIPE_SLOTS), 'pipe_p_m_pcg': ('PIPE_P_M', 'pipe', True, PIPE_SLOTS),
    'pr_pcg': ('PR', 'pr', True, PIPE_SLOTS), 'm_pcg': ('M', 'pr', True, PIPE_SLOTS),
    'pr_cg': ('PR', 'pr', False, PIPE_SLOTS), 'm_cg': ('M', 'pr', False, PIPE_SLOTS),     # (the oracle's pr_pcg / m_pcg with the identity)
    'cg_cg': ('CG_CG', 'cg', False, LAG_SLOTS), 'cg_pcg': ('CG_CG', 'cg', True, LAG_SLOTS),
    'gv_cg': ('GV', 'gv', False, LAG_SLOTS), 'gv_pcg': ('GV', 'gv', True, LAG_SLOTS),
    'hs_cg': ('HS', 'hs', False, HS_SLOTS), 'hs_pcg': ('HS', 'hs', True, HS_SLOTS),
    # the pipelined flavours without a preconditioner (another epilogue of the one-launch iteration: kEpiPipeFused / FusedP)
    'pipe_pr_cg': ('PIPE_PR', 'pipe', False, PIPE_SLOTS), 'pipe_p_cg': ('PIPE_P', 'pipe', False, PIPE_SLOTS),
}
# ... and the Meurant flavours without one: run by tests/test_trajectory_ranks.py only (METHODS parametrises other files)
ALL_METHODS = dict(METHODS, pipe_pr_m_cg=('PIPE_PR_M', 'pipe', False, PIPE_SLOTS), pipe_p_m_cg=('PIPE_P_M', 'pipe', False, PIPE_SLOTS))
ORACLE_NAME = {'pr_cg': 'pr_pcg', 'm_cg': 'm_pcg'}
CHUNKS = (1, 2, 37)          # prcg_iterate calls of mode (b), then the rest: state read at k = 3 (odd), k = 40 (even) and the end
FIELD = {'mu': 0, 'dl': 1, 'gm': 2, 'nu': 3, 'eta': 4, 'alpha': 5, 'beta': 6}


def run_oracle(method, A, b, x_true, jacobi, max_iter, dot, dot0, keep, vectors='xr', x0=None):
    """the oracle's trajectory: rows (mu, dl, gm, nu, eta, alpha, beta) per state, recorder histories, (x, r) at the states in
    `keep` (`vectors`: other fields of the oracle's state in their place, e.g. ('x', 'r', 'ut', 'wt')); `jacobi`: the callable
    the oracle takes as preconditioner= (any callable, not only a diagonal); x0: the start vector (None: zeros)"""
    rows, snaps = [], {}

    def tap(st):
        rows.append((st.mu, st.dl, st.gm, st.nu, st.eta, st.alpha, st.beta))
        if st.k in keep:
            snaps[st.k] = tuple(getattr(st, v).copy() for v in vectors)
    kw = {'preconditioner': jacobi} if ALL_METHODS[method][2] else {}
    ref = getattr(orc, ORACLE_NAME.get(method, method))(A, b, np.zeros(A.shape[0]) if x0 is None else x0, max_iter, dot=dot, dot0=dot0, square=lambda a: a * a,
                                                         callbacks=FOUR, x_true=x_true, tap=tap, **kw)
    return np.array(rows, dtype=np.float64), ref, snaps


def holds_start(start, vectors, x0, b, A, what=''):
    """the state a session holds right after begin from a start vector, bit for bit: x == x0 and r == b - A x0 (A: what the
    device multiplies with -- SciPy's product, rows summed left to right from +0.0, or LongRowOperator).  A failure here is the
    start-up's, not iteration 1's."""
    names = list(vectors)
    x, r = start[names.index('x')], start[names.index('r')]
    assert x.shape == x0.shape and np.array_equal(x, x0), f'{what}x right after begin: {int(np.count_nonzero(x != x0))} of {x0.size} entries differ from x0'
    want = b - (A @ x0)
    assert np.array_equal(r, want), \
        f'{what}r right after begin: {int(np.count_nonzero(r != want))} of {want.size} entries differ from b - A x0, worst {np.max(np.abs(r - want)):.3e}'


def run_device(L, op, variant, b, x_true, inv_diag, max_iter, recorders, *, block_jacobi=None, block_jacobi_var=None, preconditioner=None,
               vectors='xr', x0=None):
    """one session: mode (a) all four recorders, one prcg_iterate call; mode (b) the recurrence residual only, calls of CHUNKS
    and the rest, x and r (`vectors`: those state vectors) read after each.  The preconditioner is at most one of inv_diag /
    block_jacobi / block_jacobi_var / preconditioner, as DeviceCSR.begin takes them.  x0: the start vector (None: zeros); with
    one, `vectors` are also read right after begin, in either mode ('start': the state at k = 0)."""
    n = b.shape[0]
    op.begin(variant, b, np.zeros(n) if x0 is None else x0, max_iter, x_true=x_true if recorders else None, inv_diag=inv_diag, hist_mask=15 if recorders else 1,
             block_jacobi=block_jacobi, block_jacobi_var=block_jacobi_var, preconditioner=preconditioner)
    out = {'schedule': op.schedule(), 'start_layout': op.layout(), 'state': {}}
    if x0 is not None:
        out['start'] = tuple(op.get_vector(v) for v in vectors)
    if recorders:
        op.iterate(max_iter - 1)
    else:
        for chunk in CHUNKS + (max_iter,):
            op.iterate(min(chunk, max_iter - 1 - op.k))
            out['state'][int(op.k)] = tuple(op.get_vector(v) for v in vectors)
    op.sync()
    out['scalars'] = np.array([op.get_scalars(k) for k in range(max_iter)])
    out['coef'] = np.array([op.get_coefficients(k)[:2] for k in range(1, max_iter)])
    out['hist'] = op.history()
    out['layout'] = op.layout()
    return out
