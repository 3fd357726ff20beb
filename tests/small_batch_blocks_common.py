"""TEST INFRASTRUCTURE of tests/test_small_batch_block_jacobi.py: partitions, the ten systems of the big batch, the oracle stepped
under the workgroup's sum with a block-Jacobi object as `prec=`, and the device session it is compared with.  Builds on
small_batch_common.py (the nine systems, wg_dot, the stopping rule, holds_oracle)."""
import numpy as np
import scipy.sparse as sp

from small_batch_common import FLAVOUR, rule, system, vectors_of, wg_dot

FREE = 60                                # iterations of a run without thresholds: below every breakdown of TEN's table
MAX_ITER = 300
RTOL = 1e-8


def uniform(n, bs):
    """the partition 0, bs, 2 bs, ..., n with a short last block"""
    return np.minimum(np.arange(-(-n // bs) + 1, dtype=np.int64) * bs, n)


def cyclic(n):
    """sizes 1, 2, ..., 8, 1, 2, ... with the last block cut to fit"""
    ptr, k = [0], 0
    while ptr[-1] < n:
        ptr.append(min(ptr[-1] + 1 + k % 8, n))
        k += 1
    return np.array(ptr, dtype=np.int64)


# (matrix, partition): ONE batch holds them all.  Registers: bcsstk03 (112 = 37 * 3 + 1), nos4 (100), nos7 (729 = 243 * 3),
# lap32x32 (1024); LDS: 494_bus (494)
TEN = [('bcsstk03', 3), ('bcsstk03', 8), ('bcsstk03', 'cyclic'), ('nos4', 3), ('nos7', 3), ('nos7', 8), ('lap32x32', 3), ('lap32x32', 8),
       ('494_bus', 'cyclic'), ('494_bus', 8)]
NOS7_BS8 = TEN.index(('nos7', 8))


def partition(n, how):
    return cyclic(n) if how == 'cyclic' else uniform(n, how)


def ten_systems(matrices):
    """(systems [(A, b)], precs [VarBlockJacobi], matrices, mat_of): systems on one matrix share the matrix object"""
    import new_cg_variants_amd.cg_variants as cgv
    names = []
    for name, _ in TEN:
        if name not in names:
            names.append(name)
    base = {name: system(matrices, name) for name in names}
    systems = [base[name] for name, _ in TEN]
    precs = [cgv.VarBlockJacobi(A, partition(A.shape[0], how)) for (A, _), (_, how) in zip(systems, TEN)]
    return systems, precs, [base[name][0] for name in names], [names.index(name) for name, _ in TEN]


def blocks_of(precs):
    """what DeviceBatch.begin takes as block_jacobi"""
    return [(p.block_ptr, p.inv_blocks) for p in precs]


def tall_system(n, first):
    """tall_systems() of test_small_batch_jacobi.py for one (n, first): diagonal 2.5 + (i mod 7) / 7, -1 between rows i and i + 1
    for first <= i < n - 1, b_i = 1 + 0.25 sin(0.37 i)"""
    i = np.arange(n)
    link = ((i >= first) & (i < n - 1)).astype(float)[:-1]
    A = sp.csr_matrix(sp.diags([-link, 2.5 + (i % 7) / 7, -link], [-1, 0, 1]))
    A.eliminate_zeros()
    A.sort_indices()
    return A, 1 + 0.25 * np.sin(0.37 * i)


def trajectory(A, b, variant, prec, thr=None, free=FREE, cap=MAX_ITER - 1, at=(0, 1), x0=None):
    """The oracle under the workgroup's sum with `prec` (a callable), from x0 (None: zeros), in ONE pass: stepped to iteration `free`, and on --
    to `cap` at most -- until the stopping rule has fired for `thr` (None: no rule).  Returns (run, halt):
    run  -- the first `free` iterations as a session without thresholds leaves them: vec[k] for k in `at` and k = free, scalars
            rows 0..free {mu, delta, gamma, nu, rr}, coef rows 1..free, hist;
    halt -- the session stopped by the rule, in the form of small_batch_common.oracle_stopped (k_stop, status, last, at0, at,
            scalars, coef, hist), or None without thr."""
    import oracle.ne_oracle as O
    hs = variant == 'HS'
    names = vectors_of(variant)

    def row(st):
        return [st.mu, 0.0 if hs else st.dl, 0.0 if hs else st.gm, st.nu, wg_dot(st.r, st.r)]

    def snap(st):
        return {v: np.array(getattr(st, v), copy=True) for v in names}
    with np.errstate(all='ignore'):
        st = (O.hs_start if hs else O.pipe_start)(A, b, np.zeros(b.size) if x0 is None else x0, prec=prec, dot=wg_dot)
        scalars, coef, vec = [row(st)], [], {0: snap(st)}
        halt = None

        def check():
            status = 0 if thr is None else rule(st.mu, st.nu, scalars[-1][4], thr)
            if status:
                rows = np.array(scalars)
                return dict(k_stop=st.k, status=status, last=st.k, at0=vec[0], at=snap(st), scalars=rows,
                            coef=np.array(coef).reshape(-1, 3), hist=np.sqrt(rows[:, 4]))
            return None
        halt = check()
        while st.k < free or (thr is not None and halt is None and st.k < cap):
            a = st.alpha
            if hs:
                O.hs_advance(A, st, prec=prec, dot=wg_dot)
                coef.append([a, st.beta, 0.0])
            else:
                O.pipe_advance(A, st, flavour=FLAVOUR[variant], prec=prec, dot=wg_dot, square=lambda q: q * q)
                coef.append([a, st.beta, st.nu_pred])
            scalars.append(row(st))
            if st.k in at or st.k == free:
                vec[st.k] = snap(st)
            if halt is None:
                halt = check()
        rows = np.array(scalars)
        if thr is not None and halt is None:                     # ran out: the state of iteration cap
            halt = dict(k_stop=-1, status=0, last=st.k, at0=vec[0], at=snap(st), scalars=rows, coef=np.array(coef).reshape(-1, 3),
                        hist=np.sqrt(rows[:, 4]))
        run = dict(vec=vec, scalars=rows[:free + 1], coef=np.array(coef).reshape(-1, 3)[:free], hist=np.sqrt(rows[:free + 1, 4]))
        return run, halt


def run_blocks(amd, systems, variant, blocks, chunks, rr_stop=None, mat_of=None, matrices=None, max_iter=None, read=None,
               inv_diag=None, x0s=None):
    """one DeviceBatch session over `systems` [(A, b)], from x0s (one vector per system; None: zeros), begun with block_jacobi=blocks (or, blocks None, inv_diag).  One
    record per system of `read` (default: all), in the form holds_oracle takes -- the stop word, the vectors at k = 0 (at0) and
    at the end (at), every row of scalars and coefficients, the history -- plus vec[k] for every k a chunk ends on."""
    L = amd['L']
    mats = [A for A, _ in systems] if matrices is None else matrices
    batch = amd['device'].DeviceBatch(mats, mat_of)
    names = vectors_of(variant)
    total = sum(chunks)
    read = range(len(systems)) if read is None else read
    try:
        batch.begin(getattr(L, variant), [b for _, b in systems], [np.zeros(b.size) for _, b in systems] if x0s is None else x0s, max_iter or total + 1,
                    hist_mask=1,
                    block_jacobi=blocks, inv_diag=inv_diag, rr_stop=rr_stop)
        recs = {s: {'at0': {v: batch.get_vector(v, s) for v in names}} for s in read}
        for rec in recs.values():
            rec['vec'] = {0: rec['at0']}
        for c in chunks:
            batch.iterate(c)
            batch.sync()
            for s, rec in recs.items():
                rec['vec'][batch.k] = {v: batch.get_vector(v, s) for v in names}
        assert batch.k == total
        k_stop, status = batch.stops()
        for s, rec in recs.items():
            rec['k_stop'], rec['status'] = int(k_stop[s]), int(status[s])
            rec['at'] = rec['vec'][total]
            rec['scalars'] = np.array([batch.get_scalars(k, s) for k in range(total + 1)])
            rec['coef'] = np.array([batch.get_coefficients(k, s) for k in range(1, total + 1)])
            rec['hist'] = batch.history(s)['updated_residual_2_norm'][:total + 1]
        return [recs[s] for s in read]
    finally:
        batch.close()


def same_record(a, b, what=''):
    """two device records, bit for bit (NaNs equal)"""
    assert (a['k_stop'], a['status']) == (b['k_stop'], b['status']), what
    assert a['vec'].keys() == b['vec'].keys(), what
    for k in a['vec']:
        for v in a['vec'][k]:
            assert np.array_equal(a['vec'][k][v], b['vec'][k][v], equal_nan=True), (what, k, v)
    for key in ('scalars', 'coef', 'hist'):
        assert a[key].shape == b[key].shape and np.array_equal(a[key], b[key], equal_nan=True), (what, key)
