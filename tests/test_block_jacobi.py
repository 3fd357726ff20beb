"""Point-block Jacobi on the device (prcg.h: prcg_set_block_jacobi; cg_variants.BlockJacobi).

The arithmetic is fixed -- per row `acc = B[a][0] * v[0]; acc = acc + B[a][j] * v[j]`, ascending j, every product and
sum rounded -- so the device kernel, `BlockJacobi.__call__` and a plain loop must agree BIT FOR BIT, and a device
session must reproduce, entry by entry, the host-callback session that runs the same object as the caller's code (the
only way to run this preconditioner before the device path existed): both sessions launch the same kernels in the same
order around M^-1."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

METHODS = ['hs_pcg', 'cg_pcg', 'gv_pcg', 'pr_pcg', 'm_pcg', 'pipe_pr_pcg', 'pipe_p_pcg', 'pipe_pr_m_pcg', 'pipe_p_m_pcg']


@pytest.fixture(scope='module')
def amd():
    import new_cg_variants_amd.cg_variants as cgv
    import new_cg_variants_amd.callbacks as cbs
    from new_cg_variants_amd import _lib, device, problems
    return dict(cgv=cgv, cbs=cbs, L=_lib, device=device, problems=problems)


def loop_apply(inv_blocks, bs, v):
    """The contract of prcg.h, written out: blocks, rows, columns."""
    n = v.shape[0]
    out = np.zeros(n)
    for k in range(-(-n // bs)):
        cols = min(bs, n - k * bs)
        for a in range(cols):
            acc = inv_blocks[k, a, 0] * v[k * bs]
            for j in range(1, cols):
                acc = acc + inv_blocks[k, a, j] * v[k * bs + j]
            out[k * bs + a] = acc
    return out


def counting(amd, A, bs):
    """BlockJacobi whose calls are counted (the device path must never call it)."""
    class Counting(amd['cgv'].BlockJacobi):
        calls = 0

        def __call__(self, v):
            Counting.calls += 1
            return super().__call__(v)
    return Counting(A, bs), Counting


# ---------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,bs', [('bcsstk03', 1), ('bcsstk03', 2), ('bcsstk03', 3), ('bcsstk03', 4), ('bcsstk03', 7),
                                     ('bcsstk03', 8), ('nos7', 2), ('nos7', 3), ('nos7', 4)])
def test_call_is_the_contract_loop(amd, matrices, name, bs):
    A, _ = matrices[name]
    n = A.shape[0]
    P = amd['cgv'].BlockJacobi(A, bs)
    nb = -(-n // bs)
    assert P.bs == bs and P.inv_blocks.shape == (nb, bs, bs) and P.inv_blocks.dtype == np.float64
    m = n - bs * (nb - 1)
    if m < bs:          # short last block: identity around the leading m x m part
        pad = P.inv_blocks[-1].copy()
        pad[:m, :m] = np.eye(bs)[:m, :m]
        np.testing.assert_array_equal(pad, np.eye(bs))
    else:
        assert n % bs == 0
    D = A.toarray()
    for k in (0, nb // 2, nb - 1):          # the blocks ARE the inverses of the diagonal blocks
        c = min(bs, n - k * bs)
        np.testing.assert_allclose(P.inv_blocks[k, :c, :c] @ D[k * bs:k * bs + c, k * bs:k * bs + c], np.eye(c), atol=1e-9)
    rng = np.random.default_rng(5)
    for v in (rng.standard_normal(n), np.ones(n), -rng.random(n) * 1e-300):
        np.testing.assert_array_equal(P(v), loop_apply(P.inv_blocks, bs, v))


def test_fewer_iterations_than_jacobi_in_the_oracle(amd, matrices):
    from oracle import ne_oracle as orc
    A, z = matrices['bcsstk14']
    n = A.shape[0]
    its = {}
    for tag, P in (('jacobi', amd['cgv'].Jacobi(A)), ('block3', amd['cgv'].BlockJacobi(A, 3))):
        out = orc.hs_pcg(A, z['b'], np.zeros(n), 400, preconditioner=P, callbacks=['error_A_norm'], x_true=z['x_true'])
        its[tag] = orc.convergence_summary(out['error_A_norm'])[0]
    print(f'bcsstk14 hs_pcg, iterations to 1e-5: {its}')
    assert 0 < its['block3'] < its['jacobi'], its


def test_singular_block_is_refused(amd):
    D = np.diag([2.0, 3.0, 4.0, 1.0, 0.0, 0.0, 6.0])
    D[0, 1] = D[1, 0] = 1.0
    D[3, 4] = D[4, 3] = 0.5                      # couples rows 4, 5 to the rest; their own 2 x 2 diagonal block is zero
    A = sp.csr_matrix(D)
    with pytest.raises(ValueError, match='block 2 '):
        amd['cgv'].BlockJacobi(A, 2)
    with pytest.raises(ValueError, match='block 4 '):
        amd['cgv'].BlockJacobi(A, 1)             # the first zero on the diagonal
    with pytest.raises(ValueError):
        amd['cgv'].BlockJacobi(A, 9)
    D[0, 0] = np.nan
    with pytest.raises(ValueError, match='block 0 '):
        amd['cgv'].BlockJacobi(sp.csr_matrix(D), 3)


def test_entry_point_is_exported_and_refuses_a_null_handle(amd):
    L = amd['L']
    lib = L.lib()
    assert hasattr(lib, 'prcg_set_block_jacobi') and 'prcg_set_block_jacobi' in L._SIGNATURES
    assert lib.prcg_set_block_jacobi(None, 3, None) == L.EINVAL
    assert lib.prcg_version() == 1


def test_diagonal_of_hands_blocks_on_without_a_probe(amd, matrices):
    A, _ = matrices['bcsstk03']
    cgv = amd['cgv']
    P, cls = counting(amd, A, 3)
    d, fn = cgv._diagonal_of(P, A.shape[0])
    assert d is None and fn is P and cls.calls == 0
    P1, cls1 = counting(amd, A, 1)
    d, fn = cgv._diagonal_of(P1, A.shape[0])        # bs = 1 IS Jacobi
    assert fn is None and cls1.calls == 0
    np.testing.assert_array_equal(d, 1 / A.diagonal())
    assert 'BlockJacobi' in cgv.__all__


# ---------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('name,bs', [('nos7', 3), ('nos7', 4), ('bcsstk03', 3), ('bcsstk03', 8)])
@pytest.mark.parametrize('method', METHODS)
def test_device_session_equals_host_callback_session(amd, matrices, method, name, bs):
    """Same object once on the device and once as the caller's code on the host: every entry of both histories equal,
    NaN positions included."""
    A, z = matrices[name]
    n = A.shape[0]
    P, cls = counting(amd, A, bs)
    cgv = amd['cgv']
    cbs = [amd['cbs'].updated_residual_2_norm, amd['cbs'].error_A_norm]
    dev = getattr(cgv, method)(A, z['b'], np.zeros(n), 260, callbacks=cbs, x_true=z['x_true'], preconditioner=P)
    sched = cgv._operator(A, 0).schedule()
    assert sched['block_jacobi'] and not sched['fused'], sched
    assert cls.calls == 0, 'the device path called the object'
    host = getattr(cgv, method)(A, z['b'], np.zeros(n), 260, callbacks=cbs, x_true=z['x_true'], preconditioner=lambda v: P(v))
    assert cls.calls > 250 and not cgv._operator(A, 0).schedule()['block_jacobi']
    for q in ('updated_residual_2_norm', 'error_A_norm'):
        assert dev[q].shape == (260,)
        np.testing.assert_array_equal(dev[q], host[q], err_msg=f'{method}/{name}/bs={bs}: {q}')
    assert np.isfinite(dev['updated_residual_2_norm'][:20]).all() and dev['updated_residual_2_norm'][1] != 0.0


@pytest.mark.gpu
@pytest.mark.parametrize('method', ['pipe_pr_pcg', 'pipe_p_pcg', 'hs_pcg'])
def test_tilde_vectors_are_the_preconditioned_vectors(amd, matrices, method):
    """nos7, bs = 4: short last block, stride-2 sources at session start, the pair launch in the loop."""
    A, z = matrices['nos7']
    n = A.shape[0]
    P = amd['cgv'].BlockJacobi(A, 4)
    seen = []

    def spy(**env):
        if env['k'] in (0, 3, 7):
            seen.append({q: np.array(env[q]) for q in env if q.endswith('_k') and isinstance(env[q], np.ndarray)} | {'k': env['k']})
    getattr(amd['cgv'], method)(A, z['b'], np.zeros(n), 9, callbacks=[spy], preconditioner=P)
    assert amd['cgv']._operator(A, 0).schedule()['block_jacobi']
    assert [s['k'] for s in seen] == [0, 3, 7]
    for s in seen:
        k = s['k']
        if method == 'hs_pcg':
            assert np.any(s['rt_k'] != 0.0)
            np.testing.assert_array_equal(s['rt_k'], P(s['r_k']), err_msg=f'r~ at k={k}')
            continue
        assert np.any(s['ut_k'] != 0.0) and np.any(s['wt_k'] != 0.0), k
        np.testing.assert_array_equal(s['ut_k'], P(s['u_k']), err_msg=f'{method}: u~ at k={k}')
        if method == 'pipe_pr_pcg' and k > 0:
            np.testing.assert_array_equal(s['wt_k'], P(s['w_k']), err_msg=f'{method}: w~ at k={k}')


@pytest.mark.gpu
@pytest.mark.parametrize('method', METHODS)
def test_against_the_oracle(amd, matrices, method):
    """bcsstk14, bs = 3, the same object in the oracle; tolerances of test_host_callback_preconditioner."""
    from oracle import ne_oracle as orc
    A, z = matrices['bcsstk14']
    n = A.shape[0]
    P = amd['cgv'].BlockJacobi(A, 3)
    cbs = [amd['cbs'].updated_residual_2_norm, amd['cbs'].error_A_norm]
    out = getattr(amd['cgv'], method)(A, z['b'], np.zeros(n), 400, callbacks=cbs, x_true=z['x_true'], preconditioner=P)
    assert amd['cgv']._operator(A, 0).schedule()['block_jacobi']
    ref = getattr(orc, method)(A, z['b'], np.zeros(n), 400, preconditioner=P,
                               callbacks=['updated_residual_2_norm', 'error_A_norm'], x_true=z['x_true'])
    ia, aa = orc.convergence_summary(out['error_A_norm'])
    ib, ab = orc.convergence_summary(ref['error_A_norm'])
    print(f'{method}: its-to-1e-5 {ia} (oracle {ib}), log10 min error {aa:.2f} ({ab:.2f})')
    for q in ('updated_residual_2_norm', 'error_A_norm'):
        np.testing.assert_allclose(out[q][:6], ref[q][:6], rtol=1e-11, err_msg=f'{method}/{q}')
    assert ib > 0 and abs(ia - ib) <= max(2, 0.05 * ib) and abs(aa - ab) <= 1.5, ((ia, aa), (ib, ab))


@pytest.mark.gpu
@pytest.mark.parametrize('method', ['hs_pcg', 'pipe_pr_pcg'])
def test_fewer_iterations_than_jacobi_on_the_device(amd, matrices, method):
    from oracle import ne_oracle as orc
    A, z = matrices['bcsstk14']
    n = A.shape[0]
    its = {}
    for tag, P in (('jacobi', amd['cgv'].Jacobi(A)), ('block3', amd['cgv'].BlockJacobi(A, 3))):
        out = getattr(amd['cgv'], method)(A, z['b'], np.zeros(n), 400, callbacks=[amd['cbs'].error_A_norm], x_true=z['x_true'],
                                          preconditioner=P)
        assert amd['cgv']._operator(A, 0).schedule()['block_jacobi'] == (tag == 'block3')
        its[tag] = orc.convergence_summary(out['error_A_norm'])[0]
    print(f'bcsstk14 {method}, iterations to 1e-5 on the device: {its}')
    assert 0 < its['block3'] < its['jacobi'], its


@pytest.mark.gpu
def test_at_size_on_sliced_rows(amd):
    """s4b_80: n = 1,536,000, three unknowns per node, sliced-row kernels."""
    L, P_ = amd['L'], amd['problems']
    A = P_.WORKLOADS['s4b_80']['make']()
    n = A.shape[0]
    assert n == 1_536_000
    b, x0, _ = P_.reference_rhs(A, n)
    P = amd['cgv'].BlockJacobi(A, 3)
    op = amd['device'].DeviceCSR(A)
    try:
        op.begin(L.PIPE_PR, b, x0, 9, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM, block_jacobi=(P.bs, P.inv_blocks))
        sched = op.schedule()
        assert sched['sliced_rows'] and sched['block_jacobi'], sched
        op.iterate(8)
        op.sync()
        np.testing.assert_array_equal(op.get_vector('ut'), P(op.get_vector('u')))
        dev = op.history()['updated_residual_2_norm']
        op.begin(L.PIPE_PR, b, x0, 9, hist_mask=L.HIST_UPDATED_RESIDUAL_2_NORM, preconditioner=lambda v: P(v))
        assert not op.schedule()['block_jacobi']
        op.iterate(8)
        op.sync()
        host = op.history()['updated_residual_2_norm']
    finally:
        op.close()
    assert dev.shape == (9,) and np.all(dev > 0)
    np.testing.assert_array_equal(dev, host)


@pytest.mark.gpu
def test_lifecycle(amd, matrices):
    L, cgv = amd['L'], amd['cgv']
    lib = L.lib()
    A, z = matrices['nos7']
    n = A.shape[0]
    P = cgv.BlockJacobi(A, 3)
    blocks = L.f64(P.inv_blocks)
    inv_diag = L.f64(1 / A.diagonal())
    b, x0 = L.f64(z['b']), np.zeros(n)
    mask = L.HIST_UPDATED_RESIDUAL_2_NORM

    def jacobi_session(op, keep_blocks):
        if keep_blocks:      # straight through the C-ABI: DeviceCSR.begin would remove the blocks
            L.check(op._h, lib.prcg_set_block_jacobi(op._h, 3, L.ptr(blocks)))
            L.check(op._h, lib.prcg_solve_begin(op._h, L.PIPE_PR, L.ptr(b), L.ptr(x0), 60, None, L.ptr(inv_diag), mask))
            op.max_iter, op.hist_mask = 60, mask
        else:
            op.begin(L.PIPE_PR, b, x0, 60, inv_diag=inv_diag, hist_mask=mask)
        sched = op.schedule()
        op.iterate(59)
        op.sync()
        return sched, op.history()['updated_residual_2_norm']

    # blocks set AND inv_diag: Jacobi wins, on the one-launch schedule of a handle that never saw blocks
    op, fresh = amd['device'].DeviceCSR(A), amd['device'].DeviceCSR(A)
    try:
        s1, h1 = jacobi_session(op, True)
        s0, h0 = jacobi_session(fresh, False)
        assert not s1['block_jacobi'] and s1 == s0 and s0['fused'], (s1, s0)
        np.testing.assert_array_equal(h1, h0)
        # ... and the blocks are still there for the next session without inv_diag
        L.check(op._h, lib.prcg_solve_begin(op._h, L.PIPE_PR, L.ptr(b), L.ptr(x0), 60, None, None, mask))
        assert op.schedule()['block_jacobi']
        # bad block size: refused with a message, blocks untouched
        assert lib.prcg_set_block_jacobi(op._h, 9, L.ptr(blocks)) == L.EINVAL
        assert b'1..8' in lib.prcg_last_error(op._h)
        assert lib.prcg_set_block_jacobi(op._h, 0, L.ptr(blocks)) == L.EINVAL
        # a new operator drops the blocks: the next session without inv_diag is an unpreconditioned one
        op._set_matrix(A, None)
        L.check(op._h, lib.prcg_solve_begin(op._h, L.PIPE_PR, L.ptr(b), L.ptr(x0), 60, None, None, mask))
        assert not op.schedule()['block_jacobi'] and op.schedule()['fused']
        # a host callback replaces the blocks and the blocks replace a host callback: the last one set is in force
        called = []

        def host(_ctx, count, v, out):
            called.append(1)
            np.ctypeslib.as_array(out, shape=(count,))[:] = P(np.ctypeslib.as_array(v, shape=(count,)).copy())
            return 0
        fn = L.PREC_FN(host)
        L.check(op._h, lib.prcg_set_block_jacobi(op._h, 3, L.ptr(blocks)))
        L.check(op._h, lib.prcg_set_preconditioner(op._h, C.cast(fn, C.c_void_p), None))
        L.check(op._h, lib.prcg_solve_begin(op._h, L.HS, L.ptr(b), L.ptr(x0), 5, None, None, mask))
        assert not op.schedule()['block_jacobi'] and len(called) > 0
        L.check(op._h, lib.prcg_set_block_jacobi(op._h, 3, L.ptr(blocks)))
        del called[:]
        L.check(op._h, lib.prcg_solve_begin(op._h, L.HS, L.ptr(b), L.ptr(x0), 5, None, None, mask))
        assert op.schedule()['block_jacobi'] and not called
        op.begin(L.HS, b, x0, 5, preconditioner=lambda v: P(v))
        assert not op.schedule()['block_jacobi']
        with pytest.raises(AssertionError):
            op.begin(L.HS, b, x0, 5, inv_diag=inv_diag, block_jacobi=(3, blocks))
        with pytest.raises(ValueError, match='block_jacobi'):
            op.begin(L.HS, b, x0, 5, block_jacobi=(3, blocks[:-1]))
    finally:
        op.close()
        fresh.close()

    # before prcg_set_csr
    h = C.c_void_p()
    assert lib.prcg_create(C.byref(h), 0) == L.OK
    try:
        assert lib.prcg_set_block_jacobi(h, 3, L.ptr(blocks)) == L.EINVAL
        assert b'prcg_set_csr' in lib.prcg_last_error(h)
        assert lib.prcg_set_block_jacobi(h, 3, None) == L.OK          # removing nothing is fine
    finally:
        lib.prcg_destroy(h)

    # the operator cache of cg_variants reuses handles: a plain session after a block session is a plain session
    cgv.clear_operator_cache()
    cbs = [amd['cbs'].updated_residual_2_norm]
    cgv.pipe_pr_pcg(A, b, x0, 60, callbacks=cbs, preconditioner=P)
    cached = cgv._operator(A, 0)
    assert cached.schedule()['block_jacobi']
    after = cgv.pipe_pr_cg(A, b, x0, 60, callbacks=cbs)
    assert cgv._operator(A, 0) is cached
    s_after = cached.schedule()
    cgv.clear_operator_cache()
    first = cgv.pipe_pr_cg(A, b, x0, 60, callbacks=cbs)
    s_first = cgv._operator(A, 0).schedule()
    assert not s_after['block_jacobi'] and s_after == s_first, (s_after, s_first)
    np.testing.assert_array_equal(after['updated_residual_2_norm'], first['updated_residual_2_norm'])


def test_experiment_runner_refuses_an_unknown_preconditioner(amd, matrices):
    from new_cg_variants_amd.experiments import figure_run
    A, _ = matrices['bcsstk03']
    with pytest.raises(ValueError, match='unknown preconditioner'):
        figure_run.run_matrix(A, 10, 'bcsstk03', 'ilu', ['hs_pcg'], out=None)
    with pytest.raises(ValueError, match='outside 1..8'):
        figure_run.run_matrix(A, 10, 'bcsstk03', 'bjacobi9', ['hs_pcg'], out=None)


@pytest.mark.gpu
def test_experiment_runner_block_jacobi(amd, matrices, tmp_path):
    """`figure_run --block-jacobi 3` = run_matrix(preconditioner='bjacobi3'): the device session of BlockJacobi(A, 3) on the
    runner's own problem (x_true = ones / sqrt(n)), saved under <title>_bjacobi3."""
    from new_cg_variants_amd.experiments import figure_run
    A, _ = matrices['bcsstk03']
    n = A.shape[0]
    trials = figure_run.run_matrix(A, 150, 'bcsstk03', 'bjacobi3', ['hs_pcg', 'pipe_pr_pcg'], out=str(tmp_path))
    assert amd['cgv']._operator(A, 0).schedule()['block_jacobi']
    assert (tmp_path / 'bcsstk03_bjacobi3' / 'pipe_pr_pcg.npy').exists()
    x_true = np.ones(n) / np.sqrt(n)
    want = amd['cgv'].hs_pcg(A, A @ x_true, np.zeros(n), 150, callbacks=[amd['cbs'].error_A_norm], x_true=x_true,
                             preconditioner=amd['cgv'].BlockJacobi(A, 3))
    np.testing.assert_array_equal(trials['hs_pcg']['error_A_norm'], want['error_A_norm'])
