"""TEST INFRASTRUCTURE of tests/test_warm_start.py (GPU) and tests/test_warm_start_model.py (CPU): the three kinds of start vector
a session may be begun from, the tables of cases the two files share, the operators those cases run on, and the deliberately
FAULTY start-ups the CPU file shows the GPU assertions would notice.

With x0 = 0 the product A x0 is zero and r0 = b exactly: prcg_solve_begin's copy / product / subtraction, the halo exchange of x0,
the batch's x0 + voff[s] routed through slot[s] and the stop rule on row 0 run in every test and decide nothing.  The start kinds:
  random   default_rng(seed).standard_normal(n): seed 11 for a single system (as multi_rhs_common.problem), 100 + s for system s of
           a batch
  restart  the x an earlier hs_cg session ON THE SAME HANDLE holds after 20 iterations, read back with get_vector('x'); the oracle
           gets those bits.  The realistic warm start: b - A x0 cancels several digits
  solved   any x0 with b' = A @ x0, so that r0 is exactly zero -- only where a row's sum runs left to right from +0.0 (window
           operators, sliced rows, the batch), not on CSR tiles with long rows"""
import numpy as np

SEED = 11
ITERS = 60                   # iterations of every free-running case: max_iter = ITERS (trajectory bodies) / ITERS + 1 (ranks, batch)
RESTART_AFTER = 20


def random_start(n, seed=SEED):
    return np.random.default_rng(seed).standard_normal(n)


def batch_start(s, n):
    return random_start(n, 100 + s)


def restart_start(op, A, b):
    """the warm start of a restarted solve: x after RESTART_AFTER iterations of hs_cg from zeros on `op`, as the device holds it"""
    from new_cg_variants_amd import _lib as L
    op.begin(L.HS, b, np.zeros(b.size), RESTART_AFTER + 1, hist_mask=1)
    op.iterate(RESTART_AFTER)
    op.sync()
    x = op.get_vector('x')
    assert op.k == RESTART_AFTER and np.isfinite(x).all() and np.count_nonzero(x) > x.size // 2, 'the earlier session left no start vector'
    return x


# start kind -> what the trajectory bodies take as x0=: a callable (op, A, b) -> vector
STARTS = {'random': lambda op, A, b: random_start(A.shape[0]), 'restart': restart_start}


def solved_rhs(A, x0):
    """b' with r0 = b' - A x0 == 0 exactly (the device's row sums are SciPy's: left to right from +0.0)"""
    return A @ x0


# ---- the operators (name -> matrix), built without a device --------------------------------------------------------------------
def operator(name, matrices):
    from new_cg_variants_amd import problems as P
    import scipy.sparse as sp
    make = {'s3_small': lambda: P.WORKLOADS['s3_small']['make'](), 's1_small': lambda: P.WORKLOADS['s1_small']['make'](),
            'fem16': lambda: P.fem_like_3d(16, 3), 's4_short': lambda: P.irregular_standin(20000, mean_len=6),
            'fem12': lambda: P.fem_like_3d(12), 'lap2d_640x24': lambda: P.laplace_2d(640, 24)}
    if name in make:
        A = sp.csr_matrix(make[name]())
        return A, P.reference_rhs(A, A.shape[0])[0]
    A, z = matrices[name]
    return A, np.asarray(z['b'], dtype=np.float64)


# ---- a. single sessions: (method, operator of test_trajectory_oracle.py / test_trajectory_irregular.py) -----------------------
SINGLE_METHODS = ['pipe_pr_pcg', 'pipe_p_cg', 'pipe_pr_m_pcg', 'pr_pcg', 'm_cg', 'cg_cg', 'gv_pcg', 'hs_pcg']
# s3_small: Jacobi is the inverse of the band to rounding, the runs go on in rounding noise and the oracle from the random start
# breaks down for m_pcg (k = 10), pipe_pr_m_pcg (15), cg_pcg and hs_pcg (49): one method per routing family that stays clean
S3_METHODS = ['pipe_pr_pcg', 'pr_pcg', 'cg_cg', 'gv_cg', 'hs_cg']
WINDOW_OPERATORS = ['bcsstk03', 'nos7', 's3_small']                  # one tile, six tiles, 313 tiles with the dictionary stream
IRREGULAR_OPERATORS = ['fem16', 'fem16_csr', 's4_short']             # sliced rows with window codes, CSR tiles, long rows
MATRIX_OF = {'fem16_csr': 'fem16'}
SINGLE_CASES = [(m, o) for o in WINDOW_OPERATORS + IRREGULAR_OPERATORS for m in (S3_METHODS if o == 's3_small' else SINGLE_METHODS)]
STORED_TILDE_CASES = [('pipe_pr_pcg', 'fem16', 'bs3'), ('hs_pcg', 'fem16', 'bs3')]
SMALL_SOLVER_CASES = [(v, o) for v in ('PIPE_PR', 'HS') for o in ('nos7', 'bcsstk03')]       # pipe_pr_cg, hs_cg: PRCG_SMALL default
# Free-running prefix on which the one-workgroup solver and the multi-launch schedule hold 1e-12 of each other from the RANDOM start
# (tests/test_gpu_parity.py: PREFIX_FLOOR is the cold start's, 7 / 15).  Taken the same way: the reference's own loop from this
# start, its inner products re-ordered (pairwise, reversed, the device tree, four interleaved sums, exactly rounded, the
# workgroup's sum, the pair tree), leaves 1e-12 of the BLAS order at k = 7 or 8 on bcsstk03 and at k = 14 or 15 on nos7 -- one to two
# iterations earlier than from zeros (8 / 16), the start being 1e7 times farther from the solution on nos7.  The floor is one
# iteration below the earliest of them, as the cold start's is; tests/test_warm_start_model.py measures those depths and asserts
# the table against them.  Measured on MI355X (the test prints it): the one-workgroup and the multi-launch history part at k = 8 on
# bcsstk03 (both variants) and at k = 15 (pipe_pr_cg) / 14 (hs_cg) on nos7 -- the cold start's floor of 15 would not hold there.
WARM_PREFIX_FLOOR = {'bcsstk03': 6, 'nos7': 13}

# ---- b. stopped single sessions: operators of test_single_stop.py's table (window, sliced rows, CSR tiles) ---------------------
STOP_OPERATORS = ['s1_small', 'fem12', 'bcsstk14']
STOP_METHODS = ['pipe_pr_cg', 'pipe_pr_pcg']
# (max_iter, rtol): thr = (rtol ||b||_2)^2 -- relative to b, NOT to r0, whose norm from the random start is far above ||b||.
# Chosen on the CPU with the oracle under np.dot so that 0 < k_stop < max_iter - 1; the GPU test asserts that again under the
# device's tree.
STOP_RUN = {
    ('s1_small', 'pipe_pr_cg', 'random'): (60, 0.1), ('s1_small', 'pipe_pr_pcg', 'random'): (60, 0.1),
    ('fem12', 'pipe_pr_cg', 'random'): (70, 1.0), ('fem12', 'pipe_pr_pcg', 'random'): (70, 1e-2),
    ('bcsstk14', 'pipe_pr_cg', 'random'): (60, 0.25), ('bcsstk14', 'pipe_pr_pcg', 'random'): (60, 5e-3),
    # from the restart the residual is already below ||b||: smaller factors (found with the oracle's own hs_cg iterate as x0)
    ('s1_small', 'pipe_pr_cg', 'restart'): (60, 1e-2), ('s1_small', 'pipe_pr_pcg', 'restart'): (60, 1e-2),
    ('fem12', 'pipe_pr_cg', 'restart'): (60, 1e-3), ('fem12', 'pipe_pr_pcg', 'restart'): (60, 1e-3),
    ('bcsstk14', 'pipe_pr_cg', 'restart'): (60, 1e-3), ('bcsstk14', 'pipe_pr_pcg', 'restart'): (60, 1e-4),
}

# ---- c. batches: the nine systems in an order that interleaves the register and the LDS systems -------------------------------
BATCH_ORDER = [0, 5, 1, 6, 2, 7, 3, 8, 4]
BATCH_PRECS = ['none', 'jacobi', 'blocks']
BLOCK_HOW = [3, 8, 'cyclic']                                         # system s of the batch: partition BLOCK_HOW[s % 3]


def slots_of(mode):
    """prcg_batch_create's descriptor order restated: the register systems (mode 1) first, then the LDS systems, each in
    system order"""
    mode = np.asarray(mode)
    at = [int(np.count_nonzero(mode == 1)), 0]
    out = []
    for m in mode:
        out.append(at[int(m)])
        at[int(m)] += 1
    return out


def batch_systems(matrices):
    """[(name, A, b, x0)] in BATCH_ORDER, every system with its own random start"""
    from small_batch_common import NINE, system
    out = []
    for s, i in enumerate(BATCH_ORDER):
        A, b = system(matrices, NINE[i][0])
        out.append((NINE[i][0], A, b, batch_start(s, A.shape[0])))
    return out


def batch_prec(A, s, prec):
    """the oracle's prec= of system s: None, the Jacobi callable, or the VarBlockJacobi object (called: the kernel's bits)"""
    import new_cg_variants_amd.cg_variants as cgv
    import oracle.ne_oracle as O
    from small_batch_blocks_common import partition
    if prec == 'none':
        return None
    return O.jacobi(A) if prec == 'jacobi' else cgv.VarBlockJacobi(A, partition(A.shape[0], BLOCK_HOW[s % 3]))


def first_bad(scalars):
    """first row of {mu, delta, gamma, nu, rr} at which mu or nu is not finite and positive; -1: none"""
    v = np.asarray(scalars)[:, [0, 3]]
    bad = ~(np.isfinite(v) & (v > 0)).all(axis=1)
    return int(np.argmax(bad)) if bad.any() else -1


# bcsstm22 is diagonal: with Jacobi (and with any block partition, whose blocks are then diagonal) the solve is exact after one
# step and the run goes on dividing rounding noise.  (variant, preconditioner) -> the oracle's first state with a non-positive or
# non-finite mu or nu under the workgroup's sum; every other system of every batch is clean for all ITERS iterations.  Such a run
# is held as tests/test_small_batch_jacobi.py holds it from the cold start: all ITERS iterations bit for bit, NaNs equal, the
# history finite up to the breakdown.
BCSSTM22_BREAKS = {('PIPE_PR_M', 'jacobi'): 5, ('HS', 'jacobi'): 11, ('PIPE_PR_M', 'blocks'): 5, ('HS', 'blocks'): 11}

# ---- d. several ranks: (method, operator, ranks, transport) of test_trajectory_ranks.py -----------------------------------------
RANK_CASES = [('pipe_pr_cg', 's3_small', 2, t) for t in ('allreduce', 'gather', 'peer')] + \
             [('pipe_pr_pcg', 'lap2d_640x24', 3, t) for t in ('peer', 'gather_32k')] + \
             [('pipe_pr_cg', 's1_uneven', 2, 'peer'), ('hs_cg', 's1_small', 3, 'two_kernel'), ('pr_cg', 's1_small', 3, 'two_kernel')]


# ---- the faulty start-ups of tests/test_warm_start_model.py ---------------------------------------------------------------------
class FaultyFirstProduct:
    """A for the oracle, except that its FIRST product -- A x0 of the start-up -- is the one a faulty start-up would form:
    'plus'     -(A x0), so that r0 = b + A x0 (the operands of the subtraction swapped in sign)
    'no_halo'  per row block of `offsets`, the product with an x0 whose entries outside the block are zero: ghost rows of x0 that
               were never exchanged"""
    def __init__(self, A, fault, offsets=None):
        self.A, self.fault, self.offsets, self.calls, self.shape = A, fault, offsets, 0, A.shape

    def diagonal(self):
        return self.A.diagonal()

    def __matmul__(self, v):
        self.calls += 1
        if self.calls > 1:
            return self.A @ v
        if self.fault == 'plus':
            return -(self.A @ v)
        out = np.empty(self.shape[0])
        for lo, hi in zip(self.offsets[:-1], self.offsets[1:]):
            own = np.zeros_like(v)
            own[lo:hi] = v[lo:hi]
            out[lo:hi] = (self.A @ own)[lo:hi]
        return out
