"""TEST INFRASTRUCTURE shared by the batch tests (tests/test_small_batch.py, test_small_batch_jacobi.py, test_small_batch_stop.py):
the nine systems, the planner hook, the NumPy model of the workgroup's sum that the GPU tests hand to the oracle as `dot=`, and
the stopping oracle with the device session it is compared with."""
import numpy as np

from device_order import _butterfly

VARIANTS = ['PIPE_PR', 'PIPE_PR_M', 'HS']
FLAVOUR = {'PIPE_PR': 'pr', 'PIPE_PR_M': 'pr_m'}
# name -> (n, mode): 1 = matrix in registers, 0 = matrix in LDS (small_fits' rules, evaluated on the committed fixtures)
NINE = [('bcsstk03', 112, 1), ('nos4', 100, 1), ('bcsstm22', 138, 1), ('nos7', 729, 1), ('lap32x32', 1024, 1),
        ('494_bus', 494, 0), ('model_48_8_3', 48, 0), ('lap40x40', 1600, 0), ('lap33x32', 1056, 0)]
CONVERGED, BREAKDOWN = 1, 2


def system(matrices, name):
    """(A, b) of one of the nine systems: b from the fixture, ones for the Laplacians"""
    from new_cg_variants_amd import problems
    if name.startswith('lap'):
        nx, ny = (int(q) for q in name[3:].split('x'))
        A = problems.laplace_2d(nx, ny)
        return A, np.ones(A.shape[0])
    A, z = matrices[name]
    return A, np.asarray(z['b'], dtype=np.float64)


def shape_of(A):
    return A.shape[0], A.nnz, int(np.diff(A.indptr).max())


def plan(shapes, jacobi=False):
    """the planner hook; jacobi: under the preconditioned fit rule"""
    from new_cg_variants_amd import _lib as L
    n = np.array([s[0] for s in shapes], dtype=np.int64)
    nnz = np.array([s[1] for s in shapes], dtype=np.int64)
    mrl = np.array([s[2] for s in shapes], dtype=np.int32)
    mode, group = np.full(len(shapes), -1, dtype=np.int32), np.full(len(shapes), -1, dtype=np.int32)
    hook = L.lib().prcg_plan_small_batch_jacobi if jacobi else L.lib().prcg_plan_small_batch
    rc = hook(len(shapes), L.ptr(n), L.ptr(nnz), L.ptr(mrl), L.ptr(mode), L.ptr(group))
    return rc, mode, group


def slots(variant):
    return [0, 3, 4] if variant == 'HS' else [0, 1, 2, 3, 4]


def vectors_of(variant):
    return ('x', 'r', 'p', 's') if variant == 'HS' else ('x', 'r', 'p', 's', 'rt', 'st')


def names_of(variant, jacobi):
    return vectors_of(variant) if jacobi else ('x', 'r', 'p', 's')


def jacobi_of(systems):
    return [1 / A.diagonal() for A, _ in systems]


def csr_cat(mats):
    rows_off = np.concatenate([[0], np.cumsum([A.shape[0] for A in mats])]).astype(np.int64)
    nnz_off = np.concatenate([[0], np.cumsum([A.nnz for A in mats])]).astype(np.int64)
    indptr = np.concatenate([np.asarray(A.indptr, dtype=np.int32) for A in mats])
    indices = np.concatenate([np.asarray(A.indices, dtype=np.int32) for A in mats])
    data = np.concatenate([np.asarray(A.data, dtype=np.float64) for A in mats])
    return rows_off, nnz_off, indptr, indices, data


# ---- the workgroup's sum: rows tid, tid + 1024, ... in sequence; wave butterfly; the 16 wave partials by xor 8, 4, 2, 1 ----
def wg_sum(prod):
    prod = np.asarray(prod, dtype=np.float64)
    assert prod.ndim == 1 and prod.size <= 4096
    padded = np.zeros(4096)
    padded[:prod.size] = prod                                    # rows past n are never added on the device: + 0.0 is the same value
    rows = padded.reshape(4, 1024)
    acc = np.zeros(1024)
    for j in range(4):
        acc = acc + rows[j]
    v = _butterfly(acc.reshape(16, 64))                          # (16,): one partial per wave
    off = 8
    while off >= 1:
        v = v[:off] + v[off:2 * off]
        off //= 2
    return v[0]


def wg_dot(a, b):
    return wg_sum(a * b)


# ---- the stopping rule, its oracle, and the device session held to it ----
def rule(mu, nu, rr, thr):
    if rr <= thr:
        return CONVERGED
    if not (0 < mu < np.inf and 0 < nu < np.inf):
        return BREAKDOWN
    return 0


def thresholds(bs, rtol=0.0, atol=0.0):
    """thr_s = max(rtol ||b_s||_2, atol)^2, the expression of cg_variants._run_batch"""
    norms = np.array([np.linalg.norm(b) for b in bs])
    return np.maximum(rtol * norms, atol) ** 2


def oracle_stopped(A, b, variant, thr, iters, jacobi=True, x0=None):
    """the oracle under the workgroup's sum, stepped until the rule fires or `iters` iterations are done.  last: the iteration
    whose state it holds (k_stop, or iters); scalars: rows 0..last {mu, delta, gamma, nu, rr}; coef: rows 1..last.  x0: the start
    vector (None: zeros)"""
    import oracle.ne_oracle as O
    prec = O.jacobi(A) if jacobi else None
    hs = variant == 'HS'

    def row(st):
        return [st.mu, 0.0 if hs else st.dl, 0.0 if hs else st.gm, st.nu, wg_dot(st.r, st.r)]
    with np.errstate(all='ignore'):
        st = (O.hs_start if hs else O.pipe_start)(A, b, np.zeros(b.size) if x0 is None else x0, prec=prec, dot=wg_dot)
        at0 = {v: np.array(getattr(st, v), copy=True) for v in names_of(variant, jacobi)}
        scalars, coef = [row(st)], []
        k_stop, status = -1, rule(st.mu, st.nu, scalars[0][4], thr)
        if status:
            k_stop = 0
        while not status and st.k < iters:
            a = st.alpha
            if hs:
                O.hs_advance(A, st, prec=prec, dot=wg_dot)
                coef.append([a, st.beta, 0.0])
            else:
                O.pipe_advance(A, st, flavour=FLAVOUR[variant], prec=prec, dot=wg_dot, square=lambda q: q * q)
                coef.append([a, st.beta, st.nu_pred])
            scalars.append(row(st))
            status = rule(st.mu, st.nu, scalars[-1][4], thr)
            if status:
                k_stop = st.k
        scalars = np.array(scalars)
        return dict(k_stop=k_stop, status=status, last=st.k, at0=at0, at={v: np.array(getattr(st, v), copy=True) for v in at0},
                    scalars=scalars, coef=np.array(coef).reshape(-1, 3), hist=np.sqrt(scalars[:, 4]))


def run_stopping_batch(amd, systems, variant, rr_stop, chunks, jacobi=True, mat_of=None, matrices=None, read=None, x0s=None):
    """one DeviceBatch session over `systems` [(A, b)], from x0s (one vector per system; None: zeros), Jacobi or unpreconditioned, rr_stop None: no thresholds.  One
    record per system of `read` (default: all): the stop word, the vectors at k = 0 and at the end, every row of the scalars
    and coefficients, the history."""
    L = amd['L']
    mats = [A for A, _ in systems] if matrices is None else matrices
    batch = amd['device'].DeviceBatch(mats, mat_of)
    names = names_of(variant, jacobi)
    total = sum(chunks)
    read = range(len(systems)) if read is None else read
    try:
        batch.begin(getattr(L, variant), [b for _, b in systems], [np.zeros(b.size) for _, b in systems] if x0s is None else x0s, total + 1, hist_mask=1,
                    inv_diag=jacobi_of(systems) if jacobi else None, rr_stop=rr_stop)
        recs = {s: {'at0': {v: batch.get_vector(v, s) for v in names}} for s in read}
        for c in chunks:
            batch.iterate(c)
        batch.sync()
        assert batch.k == total                                  # what was launched, stopped systems or not
        k_stop, status = batch.stops()
        assert k_stop.dtype == status.dtype == np.int32 and k_stop.shape == status.shape == (len(systems),)
        for s, rec in recs.items():
            rec['k_stop'], rec['status'] = int(k_stop[s]), int(status[s])
            rec['at'] = {v: batch.get_vector(v, s) for v in names}
            rec['scalars'] = np.array([batch.get_scalars(k, s) for k in range(total + 1)])
            rec['coef'] = np.array([batch.get_coefficients(k, s) for k in range(1, total + 1)])
            rec['hist'] = batch.history(s)['updated_residual_2_norm']
        return [recs[s] for s in read]
    finally:
        batch.close()


def holds_oracle(rec, want, variant, total, what=''):
    """a device record of `total` launched iterations against oracle_stopped"""
    idx, ncoef, last = slots(variant), 2 if variant == 'HS' else 3, want['last']
    assert (rec['k_stop'], rec['status']) == (want['k_stop'], want['status']), (what, 'stop word', rec['k_stop'], rec['status'])
    assert last == (want['k_stop'] if want['status'] else total)
    for v in want['at']:
        assert np.array_equal(rec['at0'][v], want['at0'][v]), (what, 'k = 0', v)
        assert np.array_equal(rec['at'][v], want['at'][v]), (what, 'at the stop', v)
    assert rec['scalars'].shape == (total + 1, 8) and rec['coef'].shape == (total, 3) and rec['hist'].shape == (total + 1,)
    assert np.array_equal(rec['scalars'][:last + 1, idx], want['scalars'][:, idx]), (what, 'scalars')
    assert np.array_equal(rec['coef'][:last, :ncoef], want['coef'][:, :ncoef]), (what, 'coefficients')
    assert np.array_equal(rec['scalars'][last + 1:], np.zeros((total - last, 8))), (what, 'scalar rows beyond the stop')
    assert np.array_equal(rec['coef'][last:], np.zeros((total - last, 3))), (what, 'coefficient rows beyond the stop')
    assert np.array_equal(rec['hist'][:last + 1], want['hist']), (what, 'history')
    assert np.array_equal(rec['hist'][last + 1:], np.zeros(total - last)), (what, 'history beyond the stop')
