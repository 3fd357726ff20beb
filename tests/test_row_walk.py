"""Row walk of the window kernels (DESIGN.md section 4, row-per-lane window kernels, step 3): the cached walks read a tile's
window entries in batches behind ONE wave-uniform branch per tile on the slot count, 1 ... 16.  Every slot count, every walk
(uniform rows, the two cached lane-by-lane walks, the pattern walks) and the paths that lead into them (`fill`: the wave's
first tile of an image; `same_cur`: the same image again) are held to the bars the walks had before: products equal SciPy's
csr_matvec bit for bit; solver steps equal the project's own multi-launch schedules.

Operators: the ex2b band with half bandwidth 0 ... 7 (1 ... 15 slots) and one asymmetric band of 16 diagonals (the row
cache's full 16 slots), each with kappa = 1 (constant diagonals: pattern tiles) and kappa = 1e6 (dictionary kernel with row
cache; only the last rows' diagonal entries differ, so the last tiles hold up to 65 values and take the dictionary walk).
Sizes: 64*5 + 37 rows (edge tiles at both ends, a partial last tile, one tile per wave) and 2^19 + 37 rows (more tiles than
resident waves: a wave meets the same image twice in a row).

NaN: a NaN a product creates has no agreed payload (x86 sets the sign bit, the GPU does not), so NaNs must sit at the same
places and every other element must have the same bits."""
import numpy as np
import pytest
import scipy.sparse as sp

pytestmark = pytest.mark.gpu

N_SMALL = 64 * 5 + 37
N_LARGE = 2 ** 19 + 37
BANDS = list(range(8)) + ['asym16', 'three', 'negzero']
STEPS = 8


@pytest.fixture(scope='module')
def amd():
    from new_cg_variants_amd import _lib, device, problems
    return dict(L=_lib, device=device, problems=problems)


def ex2b_diagonal(n, kappa, rho=0.95):
    i = np.arange(n, dtype=np.float64)
    return 1.0 + (i / (n - 1.0)) * (kappa - 1.0) * np.power(rho, (n - 1.0) - i)


def band_from_offsets(n, offsets, values, kappa):
    """CSR band with sorted columns; off-diagonal `values[q]` on diagonal `offsets[q]` (explicit zeros are KEPT), the ex2b
    diagonal on offset 0."""
    offsets = np.asarray(offsets, dtype=np.int64)
    I = np.arange(n, dtype=np.int64)[:, None]
    J = I + offsets[None, :]
    valid = (J >= 0) & (J < n)
    V = np.tile(np.asarray(values, dtype=np.float64)[None, :], (n, 1))
    V[:, int(np.nonzero(offsets == 0)[0][0])] = ex2b_diagonal(n, kappa)
    counts = valid.sum(axis=1)
    indptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return sp.csr_matrix((V[valid], J[valid].astype(np.int32), indptr), shape=(n, n))


_OPERATORS = {}


def operator(P, band, kappa, n):
    key = (band, kappa, n)
    if key not in _OPERATORS:
        if band == 'asym16':
            # 16 diagonals, offsets -8 ... 7: the row cache's full 16 slots
            offs = list(range(-8, 8))
            A = sp.diags([ex2b_diagonal(n, kappa)[:n - abs(o)] if o == 0 else np.full(n - abs(o), 1e-4) for o in offs], offs,
                         shape=(n, n), format='csr', dtype=np.float64)
            A.sort_indices()
        elif band == 'three':
            # three distinct off-diagonal values: four values per tile with the diagonal's (more than a select covers)
            offs = list(range(-7, 8))
            A = band_from_offsets(n, offs, [(1e-4, 2e-4, 3e-4)[abs(o) % 3] for o in offs], kappa)
        elif band == 'negzero':
            # stored -0.0 on four diagonals: (-0.0) * x keeps its sign, (-0.0) * inf is a NaN
            offs = list(range(-7, 8))
            A = band_from_offsets(n, offs, [-0.0 if abs(o) in (2, 5) else 1e-4 for o in offs], kappa)
        else:
            A = P.banded_ex2b(n, band, kappa=kappa)
        assert A.has_sorted_indices
        _OPERATORS[key] = A
    return _OPERATORS[key]


def half_bandwidth(band):
    return band if isinstance(band, int) else (8 if band == 'asym16' else 7)


def same_bits(a, b):
    """Same NaN positions, same 64-bit patterns everywhere else."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def input_vectors(n, k):
    """A plain pair of vectors and a pair holding -0.0, inf and nan in the rows next to the band's edges and next to tile
    boundaries (every row within k of such an entry sees it)."""
    rng = np.random.default_rng(1234 + 17 * k + n % 1000)
    plain = rng.standard_normal((n, 2))
    hard = rng.standard_normal((n, 2))
    last = n - 1
    for col, (zero_at, inf_at, nan_at) in enumerate((((0, 64, last), (k + 1, 64 * 3 - 1), (last - k - 1,)),
                                                     ((k, 63, last - k), (last - 1,), (k + 2, 64 * 2)))):
        hard[list(zero_at), col] = -0.0
        hard[list(inf_at), col] = np.inf
        hard[list(nan_at), col] = np.nan
    hard[64 * 4 + 1, 0] = -np.inf
    return plain, hard


def reference_products(A, X):
    """SciPy's csr_matvec, one column at a time (what `A @ v` runs in the reference)."""
    with np.errstate(all='ignore'):
        return np.stack([A @ np.ascontiguousarray(X[:, q]) for q in range(X.shape[1])], axis=1)


@pytest.mark.parametrize('n', [N_SMALL, N_LARGE])
@pytest.mark.parametrize('kappa', [1.0, 1e6])
@pytest.mark.parametrize('band', BANDS)
def test_products_equal_scipy(amd, band, kappa, n):
    """matvec and matmat2 against SciPy, bit for bit, on plain and on hard input vectors; on the constant-diagonal bands also
    through the stream geometries (PRCG_WIN_PAT=0)."""
    P = amd['problems']
    A = operator(P, band, kappa, n)
    plain, hard = input_vectors(n, half_bandwidth(band))
    want = {name: reference_products(A, X) for name, X in (('plain', plain), ('hard', hard))}
    for knobs in ({}, {'PRCG_WIN_PAT': '0'}) if kappa == 1.0 else ({},):
        op = amd['device'].DeviceCSR(A, knobs=knobs)
        for name, X in (('plain', plain), ('hard', hard)):
            for q in range(2):
                y, _ = op.matvec(np.ascontiguousarray(X[:, q]))
                assert same_bits(y, want[name][:, q]), (knobs, name, q)
            WU, _ = op.matmat2(X)
            assert same_bits(WU, want[name]), (knobs, name)
        b, x0, _ = P.reference_rhs(A, n)
        op.begin(amd['L'].PIPE_PR, b, x0, 4)
        s = op.schedule()
        assert s['window'], s
        assert s['pattern'] == (kappa == 1.0 and not knobs), s
        if kappa != 1.0:
            assert s['value_dict'] and s['col_bytes'] in (1, 2), s      # (narrow bands take the geometry with 2-byte indices)
        op.close()


def forced_steps(ops, L, variant, b, n, inv_diag, stored, steps=STEPS):
    """Teacher-forced single steps: ops[0] gets ops[1]'s state, both step once.  Returns the worst relative deviation of the
    scalars (of those that are finite and not zero; the others must be equal); vectors and coefficients must agree bit for bit."""
    for op in ops:
        op.begin(getattr(L, variant), b, np.zeros(n), steps + 2, inv_diag=inv_diag)
    worst = 0.0
    for k in range(steps):
        for v in stored:
            ops[0].set_vector(v, ops[1].get_vector(v))
        ops[0].set_scalars(k, ops[1].get_scalars(k))
        ops[0].set_iteration(k)
        for op in ops:
            op.iterate(1)
        for v in stored:
            assert same_bits(ops[0].get_vector(v), ops[1].get_vector(v)), (variant, k, v)
        a, c = ops[0].get_scalars(k + 1)[:5], ops[1].get_scalars(k + 1)[:5]
        # (the identity -- half bandwidth 0, kappa = 1 -- converges in one step: zeros, then 0 / 0; such entries must match exactly)
        rel = np.isfinite(c) & (c != 0)
        assert same_bits(a[~rel], c[~rel]), (variant, k, a, c)
        if rel.any():
            worst = max(worst, float(np.max(np.abs(a[rel] - c[rel]) / np.abs(c[rel]))))
        assert same_bits(ops[0].get_coefficients(k + 1), ops[1].get_coefficients(k + 1)), (variant, k)
    return worst


# every operator at both kappas at the small size (every slot count in every solver instantiation against an independent
# schedule); the large size -- the same image twice in a row -- for slot counts 1, 9, 15, 16 and the four-value table
SOLVER_CASES = ([(band, kappa, N_SMALL) for band in BANDS for kappa in (1.0, 1e6)] +
                [(0, 1e6, N_LARGE), (4, 1e6, N_LARGE), (7, 1e6, N_LARGE), (7, 1.0, N_LARGE), ('asym16', 1e6, N_LARGE),
                 ('asym16', 1.0, N_LARGE), ('three', 1e6, N_LARGE)])


@pytest.mark.parametrize('band,kappa,n', SOLVER_CASES)
def test_pipelined_one_launch_against_two_kernels(amd, band, kappa, n):
    """pipe_pr_cg and pipe_pr_pcg (Jacobi), 8 forced steps of the one-launch iteration against the same session with
    PRCG_FUSED=0: vectors bit for bit, scalars <= 1e-12 relative (one-launch vs two-kernel schedule).
    (8 iterations of a conjugate-gradient recurrence on the asymmetric band are arithmetic like any other: nothing breaks down)"""
    L, P = amd['L'], amd['problems']
    A = operator(P, band, kappa, n)
    b = P.reference_rhs(A, n)[0]
    ops = [amd['device'].DeviceCSR(A, knobs={'PRCG_FUSED': f, 'PRCG_SMALL': '0'}) for f in ('1', '0')]
    for inv_diag in (None, 1 / A.diagonal()):
        stored = ['x', 'r', 'p', 's'] + (['rt', 'st'] if inv_diag is not None else [])
        worst = forced_steps(ops, L, 'PIPE_PR', b, n, inv_diag, stored)
        assert ops[0].schedule()['fused'] and ops[0].schedule()['window'] and not ops[1].schedule()['fused']
        print(f'{band}/{kappa:g}/{n} pipe_pr_{"pcg" if inv_diag is not None else "cg"}: worst scalar deviation {worst:.2e}')
        assert worst <= 1e-12, worst
    for op in ops:
        op.close()


@pytest.mark.parametrize('band,kappa,n', SOLVER_CASES)
def test_split_calls_with_and_without_deferred_store(amd, band, kappa, n):
    """pipe_pr_cg as iterate(1), iterate(2), iterate(5) with PRCG_XP_DEFER at 1 and at 0: every vector, scalar and coefficient
    bit for bit after every call (the deferred store changes no rounding)."""
    L, P = amd['L'], amd['problems']
    A = operator(P, band, kappa, n)
    b, x0, _ = P.reference_rhs(A, n)
    ops = [amd['device'].DeviceCSR(A, knobs={'PRCG_SMALL': '0', 'PRCG_XP_DEFER': d}) for d in ('1', '0')]
    for op in ops:
        op.begin(L.PIPE_PR, b, x0, STEPS + 1, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM)
    assert ops[0].schedule()['xp_deferred'] and not ops[1].schedule()['xp_deferred']
    k = 0
    for call in (1, 2, 5):
        for op in ops:
            op.iterate(call)
        for v in ('x', 'p', 'r', 's'):
            assert same_bits(ops[0].get_vector(v), ops[1].get_vector(v)), (k, call, v)
        for kk in range(k, k + call + 1):
            assert same_bits(ops[0].get_scalars(kk), ops[1].get_scalars(kk)), (k, call, kk)
        for kk in range(k + 1, k + call + 1):
            assert same_bits(ops[0].get_coefficients(kk), ops[1].get_coefficients(kk)), (k, call, kk)
        k += call
    assert ops[0].k == STEPS and ops[1].k == STEPS
    for op in ops:
        op.close()


@pytest.mark.parametrize('band,kappa,n', SOLVER_CASES)
def test_hestenes_stiefel_and_predict_and_recompute(amd, band, kappa, n):
    """hs_cg: 8 free-running iterations against the five-launch schedule (PRCG_FUSED=0), same summation order: every vector,
    scalar and coefficient bit for bit.  pr_cg: 8 forced steps of the one-launch iteration against the four-launch schedule:
    vectors bit for bit, scalars <= 1e-12 relative."""
    L, P = amd['L'], amd['problems']
    A = operator(P, band, kappa, n)
    b = P.reference_rhs(A, n)[0]
    ops = [amd['device'].DeviceCSR(A, knobs={'PRCG_FUSED': f, 'PRCG_SMALL': '0'}) for f in ('1', '0')]
    for op in ops:
        op.begin(L.HS, b, np.zeros(n), STEPS + 1)
    assert ops[0].schedule()['fused'] and ops[0].schedule()['window'] and not ops[1].schedule()['fused']
    k = 0
    for call in (1, 2, 5):
        for op in ops:
            op.iterate(call)
        k += call
        for v in ('x', 'r', 'p', 's'):
            assert same_bits(ops[0].get_vector(v), ops[1].get_vector(v)), (k, v)
        for kk in range(k - call, k + 1):
            assert same_bits(ops[0].get_scalars(kk)[:5], ops[1].get_scalars(kk)[:5]), (k, kk)
            if kk >= 1:
                assert same_bits(ops[0].get_coefficients(kk)[:2], ops[1].get_coefficients(kk)[:2]), (k, kk)
    worst = forced_steps(ops, L, 'PR', b, n, None, ['x', 'r', 'p', 's'])
    assert ops[0].schedule()['fused'] and ops[0].schedule()['window'] and not ops[1].schedule()['fused']
    print(f'{band}/{kappa:g}/{n} pr_cg: worst scalar deviation {worst:.2e}')
    assert worst <= 1e-12, worst
    for op in ops:
        op.close()


# Bands whose pattern tiles and stream tiles give the launch the same layout (grid, waves per workgroup, tile table): the inner
# products are then summed in the same order and free-running sessions agree bit for bit.  Half bandwidths 0 ... 4 take the
# stream geometry with 2-byte window indices, whose launch has another grid: their inner products differ in the last bits
# whatever the row walk does (profiles/row_walk.md C), so their vectors can be compared from identical state only.
SAME_LAYOUT = (5, 6, 7, 'asym16')


@pytest.mark.parametrize('n', [N_SMALL, N_LARGE])
@pytest.mark.parametrize('band', [0, 1, 2, 3, 4, 5, 6, 7, 'asym16'])
def test_pattern_and_stream_kernels_agree(amd, band, n):
    """The constant-diagonal bands through pattern tiles (default) and through the stream geometries (PRCG_WIN_PAT=0), 8
    iterations of pipe_pr_cg.  Every band: 8 steps, each from identical state, vectors bit for bit and scalars <= 1e-12
    relative.  The bands of SAME_LAYOUT -- asserted, not assumed -- also 8 free-running iterations, vectors bit for bit."""
    L, P = amd['L'], amd['problems']
    A = operator(P, band, 1.0, n)
    b, x0, _ = P.reference_rhs(A, n)
    ops = [amd['device'].DeviceCSR(A, knobs=dict(PRCG_SMALL='0', **extra)) for extra in ({}, {'PRCG_WIN_PAT': '0'})]
    worst = forced_steps(ops, L, 'PIPE_PR', b, n, None, ['x', 'r', 'p', 's'])
    assert ops[0].schedule()['pattern'] and not ops[1].schedule()['pattern']
    assert worst <= 1e-12, worst
    for op in ops:
        op.begin(L.PIPE_PR, b, x0, STEPS + 1)
        op.iterate(STEPS)
    lay = [op.layout() for op in ops]
    same_layout = all(np.array_equal(lay[0][q], lay[1][q]) for q in ('grid', 'waves_per_block', 'tiles'))
    print(f'{band}/{n}: pattern vs stream, worst scalar deviation {worst:.2e}, same layout {same_layout}, '
          f'stream col_bytes {ops[1].schedule()["col_bytes"]}, grids {lay[0]["grid"]} x {lay[0]["waves_per_block"]} / {lay[1]["grid"]} x {lay[1]["waves_per_block"]}')
    assert same_layout == (band in SAME_LAYOUT), (band, n, lay[0]['grid'], lay[1]['grid'])
    if same_layout:
        for v in ('x', 'p', 'r', 's'):
            assert same_bits(ops[0].get_vector(v), ops[1].get_vector(v)), v
    for op in ops:
        op.close()
