"""Host-side owner of one libprcg handle: one GPU, one row block, one rank.

This is the thin layer between SciPy CSR arrays and the C-ABI (include/prcg.h); every
numerical operation happens in the HIP kernels behind it.
"""
import contextlib
import ctypes as C
import os
import sys

import numpy as np

from . import _lib as L


@contextlib.contextmanager
def _stdout_to_stderr():
    """RCCL prints a version banner on fd 1 when a communicator is created; a program
    whose stdout is a protocol (bench.py prints exactly one JSON line) must not see it."""
    sys.stdout.flush()
    saved = os.dup(1)
    try:
        os.dup2(2, 1)
        yield
    finally:
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(saved)


class DeviceCSR:
    """A CSR row block resident on one MI355X.

    ``A`` is what the reference passes around as ``A``: a ``scipy.sparse`` CSR matrix
    (numerical_experiments/figure_gen.py:350).  For a multi-rank run ``A`` is the rank's
    row block with LOCAL column numbering and ``halo`` the plan produced by
    ``partition.plan_halo`` (columns >= n_rows are ghosts).
    """

    def __init__(self, A, device=0, comm_init=None, halo=None, knobs=None, world=None):
        """knobs: dict of PRCG_* experiment switches for THIS handle (prcg_set_option), e.g.
        {'PRCG_FUSED': '0'} keeps the two-kernel schedule on one GPU.  The process environment
        is not touched."""
        self._h = C.c_void_p()
        self._lib = L.lib()
        self.device = int(device)
        rc = self._lib.prcg_create(C.byref(self._h), int(device))
        if rc != L.OK:
            msg = self._lib.prcg_last_error(None)
            self._h = C.c_void_p()
            raise L.PrcgError(rc, msg.decode() if msg else '?')
        for k, v in (knobs or {}).items():
            self._check(self._lib.prcg_set_option(self._h, str(k).encode(), str(v).encode()))
        self.rank, self.nranks = 0, 1
        if comm_init is not None:
            rank, nranks, uid, path = comm_init      # uid: 128 or 256 bytes (one or two RCCL ids)
            ids = np.frombuffer(uid, dtype=np.uint8).copy()
            assert ids.size in (128, 256)
            with _stdout_to_stderr():
                self._check(self._lib.prcg_comm_init(self._h, path.encode() if path else None, rank, nranks,
                                                     L.ptr(ids), ids.size // 128))
            self.rank, self.nranks = rank, nranks
        elif world is not None:        # rank / world size without a communicator (prcg.h: prcg_world_init; peer-exchange plumbing only)
            self._check(self._lib.prcg_world_init(self._h, int(world[0]), int(world[1])))
            self.rank, self.nranks = int(world[0]), int(world[1])
        self._set_matrix(A, halo)

    # -- plumbing ---------------------------------------------------------------------
    def _check(self, rc):
        L.check(self._h, rc)

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            self._lib.prcg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _set_matrix(self, A, halo):
        if not hasattr(A, 'indptr'):
            raise TypeError('A must be a scipy.sparse CSR matrix/array')
        if A.format != 'csr':
            A = A.tocsr()
        if A.dtype != np.float64:
            raise TypeError(f'fp64 only (got {A.dtype}); the reference works in double precision')
        n_rows, n_cols = A.shape
        n_ghost = n_cols - n_rows
        if n_ghost < 0:
            raise ValueError('row block must have at least n_rows columns (local numbering)')
        indptr = np.ascontiguousarray(A.indptr)
        is64 = indptr.dtype == np.int64
        if not is64:
            indptr = np.ascontiguousarray(indptr, dtype=np.int32)
        indices = np.ascontiguousarray(A.indices, dtype=np.int32)
        data = np.ascontiguousarray(A.data, dtype=np.float64)
        self.n, self.n_ghost, self.nnz = int(n_rows), int(n_ghost), int(A.nnz)
        self._no_blocks()                            # prcg_set_csr drops block-Jacobi blocks
        self._check(self._lib.prcg_set_csr(self._h, self.n, self.n_ghost, self.nnz, L.ptr(indptr), int(is64),
                                           L.ptr(indices), L.ptr(data)))
        self.halo = halo
        if halo is not None:
            peers = np.ascontiguousarray(halo['peers'], dtype=np.int32)
            send_ptr = np.ascontiguousarray(halo['send_ptr'], dtype=np.int64)
            send_idx = np.ascontiguousarray(halo['send_idx'], dtype=np.int32)
            recv_ptr = np.ascontiguousarray(halo['recv_ptr'], dtype=np.int64)
            self._check(self._lib.prcg_set_halo(self._h, len(peers), L.ptr(peers), L.ptr(send_ptr),
                                                L.ptr(send_idx), L.ptr(recv_ptr)))

    # -- new values on the same pattern (prcg.h: prcg_update_values) -----------------------------------
    def values_route(self):
        """How update_values serves the operator now on the handle: 'in_place' (no encoding holds values: no host planning)
        or 'replanned' (value dictionary or pattern tiles)."""
        route = int(self._lib.prcg_values_route(self._h))
        if route not in (0, 1):
            raise RuntimeError('prcg_values_route: the handle has no operator')
        return ('in_place', 'replanned')[route]

    def update_values(self, data):
        """New values for the nonzeros of the matrix this handle was built from -- same shape, indptr and indices, the
        caller's promise -- instead of a second DeviceCSR(A).  ``data``: nnz float64 values in the order of that matrix's CSR
        arrays, as an array (or CPU tensor), or as a CUDA torch tensor, which is read where it lies: it must be float64,
        contiguous, of nnz elements and on the handle's device (ValueError otherwise), and its memory must belong to the HIP
        runtime libprcg.so is bound to, i.e. torch was imported before the library was loaded (the library refuses a pointer
        its runtime does not know).  torch's current stream on that device is synchronised first.
        Returns the route taken, 'in_place' or 'replanned' (values_route).  An open session ends; options, a host-callback
        preconditioner and block-Jacobi blocks stay in force."""
        if type(data).__module__.split('.')[0] == 'torch' and hasattr(data, 'is_cuda'):
            if data.is_cuda:
                import torch
                if data.dtype != torch.float64:
                    raise ValueError(f'update_values: fp64 only (got a {data.dtype} tensor)')
                if data.numel() != self.nnz:
                    raise ValueError(f'update_values: the operator has {self.nnz} nonzeros, the tensor {data.numel()} elements')
                if not data.is_contiguous():
                    raise ValueError('update_values: the tensor must be contiguous (the values are read where they lie)')
                if data.device.index != self.device:
                    raise ValueError(f'update_values: the tensor lies on {data.device}, the handle on GPU {self.device}')
                torch.cuda.current_stream(data.device).synchronize()
                route = self.values_route()
                self._check(self._lib.prcg_update_values(self._h, C.c_void_p(data.data_ptr()), 1))
                self._bj_built = self._bjv_built = None      # the blocks stay, frozen: no longer those of the current values
                return route
            data = data.detach().numpy()
        data = np.asarray(data)
        if data.dtype != np.float64:
            raise ValueError(f'update_values: fp64 only (got {data.dtype})')
        if data.size != self.nnz or data.ndim != 1:
            raise ValueError(f'update_values: the operator has {self.nnz} nonzeros, the array has shape {data.shape}')
        data = np.ascontiguousarray(data)
        route = self.values_route()
        self._check(self._lib.prcg_update_values(self._h, L.ptr(data), 0))
        self._bj_built = self._bjv_built = None      # the blocks stay, frozen: no longer those of the current values
        return route

    # -- point-block Jacobi: the blocks on the handle (prcg.h: prcg_set_block_jacobi / prcg_build_block_jacobi) ----------
    _bj_bs = None        # block size of the blocks this wrapper put on the handle (None: none)
    _bj_built = None     # ... and, when they were BUILT from the operator's current values, that block size again

    _bjv_ptr = None      # partition of the VARIABLE-size blocks this wrapper put on the handle (None: none; then _bj_bs is None)
    _bjv_built = None    # ... and, when they were BUILT from the operator's current values, that partition again

    def _no_blocks(self):
        self._bj_bs = self._bj_built = self._bjv_ptr = self._bjv_built = None

    # -- ... with variable block sizes (prcg.h: prcg_set_block_jacobi_var / prcg_build_block_jacobi_var) ------------------
    def _partition(self, block_ptr, who):
        """block_ptr as a contiguous int64 array; the library checks what it says (and names the reason of a refusal)"""
        ptr = np.ascontiguousarray(block_ptr, dtype=np.int64)
        if ptr.ndim != 1 or ptr.size < 1:
            raise ValueError(f'{who}: block_ptr must be a one-dimensional array of nb + 1 entries, got shape {ptr.shape}')
        return ptr

    def set_block_jacobi_var(self, block_ptr, inv_blocks):
        """Put the caller's inverses of variable-size diagonal blocks on the handle (prcg.h: prcg_set_block_jacobi_var): block k
        owns rows block_ptr[k] .. block_ptr[k+1]-1, every size in 1..8; inv_blocks packed, block k as m_k x m_k row-major at
        offset sum of m_q^2, q < k.  inv_blocks None removes whatever blocks are set.  A partition the library refuses leaves
        the blocks set before in force (PrcgError with the reason)."""
        if inv_blocks is None:
            self._check(self._lib.prcg_set_block_jacobi_var(self._h, 0, None, None))
            self._no_blocks()
            return
        ptr = self._partition(block_ptr, 'set_block_jacobi_var')
        blocks = L.f64(inv_blocks).reshape(-1)
        want = int((np.diff(ptr) ** 2).sum())
        if blocks.size != want:
            raise ValueError(f'set_block_jacobi_var: the partition needs {want} packed doubles (sum of m_k^2), inv_blocks has {blocks.size}')
        self._check(self._lib.prcg_set_block_jacobi_var(self._h, ptr.size - 1, L.ptr(ptr), L.ptr(blocks)))
        self._no_blocks()
        self._bjv_ptr = ptr.copy()

    def build_block_jacobi_var(self, block_ptr):
        """Build the inverses of the diagonal blocks of the partition ON THE DEVICE from the operator's current values (prcg.h:
        prcg_build_block_jacobi_var) and put them in force.  Valid again after every update_values.  ValueError with the
        library's text if a block is singular or not finite (the handle is then left without blocks); any other refusal is
        a PrcgError and leaves the handle as it was."""
        ptr = self._partition(block_ptr, 'build_block_jacobi_var')
        bad = C.c_int64(-1)
        rc = self._lib.prcg_build_block_jacobi_var(self._h, ptr.size - 1, L.ptr(ptr), C.byref(bad))
        if rc == L.EINVAL and bad.value >= 0:
            self._no_blocks()
            raise ValueError(self._lib.prcg_last_error(self._h).decode())
        self._check(rc)
        self._no_blocks()
        self._bjv_ptr = self._bjv_built = ptr.copy()

    def get_block_jacobi_var(self, block_ptr=None):
        """The variable-size blocks now on the handle, packed (prcg.h: prcg_get_block_jacobi_var).  block_ptr: the partition
        they were set with -- known to this object when it set them itself, to be passed when the C-ABI was called around it."""
        ptr = self._bjv_ptr if block_ptr is None else self._partition(block_ptr, 'get_block_jacobi_var')
        out = np.zeros(self.n * 8 + 8)               # room for any partition: a row has at most 8 entries
        self._check(self._lib.prcg_get_block_jacobi_var(self._h, L.ptr(out)))       # (refuses without variable blocks)
        if ptr is None:
            raise ValueError('get_block_jacobi_var: this object has set no variable blocks; pass block_ptr= if the C-ABI was called directly')
        return out[:int((np.diff(ptr) ** 2).sum())].copy()

    def set_block_jacobi(self, bs, inv_blocks):
        """Put the caller's inverses on the handle (prcg.h: prcg_set_block_jacobi): inv_blocks of shape (ceil(n/bs), bs, bs);
        inv_blocks None removes whatever blocks are set."""
        if inv_blocks is None:
            self._check(self._lib.prcg_set_block_jacobi(self._h, 0, None))
            self._no_blocks()
            return
        bs, blocks = int(bs), L.f64(inv_blocks)
        if not 1 <= bs <= 8 or blocks.shape != (-(-self.n // bs), bs, bs):
            raise ValueError(f'block_jacobi: need 1 <= bs <= 8 and inv_blocks of shape (ceil(n/bs), bs, bs); got bs={bs}, {blocks.shape}')
        self._no_blocks()
        self._check(self._lib.prcg_set_block_jacobi(self._h, bs, L.ptr(blocks)))
        self._bj_bs = bs

    def build_block_jacobi(self, bs):
        """Build the inverses of the bs x bs diagonal blocks ON THE DEVICE from the operator's current values (prcg.h:
        prcg_build_block_jacobi: one kernel pass, no host pass over the matrix, no upload) and put them in force, as
        set_block_jacobi would.  Valid again after every update_values.  ValueError with the library's text if a block is
        singular or not finite (the handle is then left without blocks); any other refusal is a PrcgError."""
        bad = C.c_int64(-1)
        rc = self._lib.prcg_build_block_jacobi(self._h, int(bs), C.byref(bad))
        if rc == L.EINVAL and bad.value >= 0:
            self._no_blocks()
            raise ValueError(self._lib.prcg_last_error(self._h).decode())
        self._check(rc)
        self._no_blocks()                            # (they replace variable-size blocks too)
        self._bj_bs = self._bj_built = int(bs)

    def get_block_jacobi(self, bs=None):
        """The blocks now on the handle as (ceil(n/bs), bs, bs) (prcg.h: prcg_get_block_jacobi), a short last block as its leading
        m x m part inside an identity.  bs: the block size they were set with -- known to this object when it set them itself
        (begin, set_block_jacobi, build_block_jacobi), to be passed when the C-ABI was called around it."""
        bs = self._bj_bs if bs is None else int(bs)
        if bs is None:
            raise ValueError('get_block_jacobi: this object has set no blocks; pass bs= if the C-ABI was called directly')
        out = np.zeros((self.n + 8) * 8)             # room for any bs in 1..8
        self._check(self._lib.prcg_get_block_jacobi(self._h, L.ptr(out)))
        nb = -(-self.n // bs)
        return out[:nb * bs * bs].reshape(nb, bs, bs).copy()

    # -- direct peer exchange (prcg.h: prcg_peer_setup / prcg_peer_connect) ------------------------------
    def peer_setup(self, max_ghost_any_rank):
        """Allocate this rank's exchange buffer; returns (64-byte IPC handle, device address)."""
        handle = np.zeros(64, dtype=np.uint8)
        ptr = C.c_void_p()
        self._check(self._lib.prcg_peer_setup(self._h, int(max_ghost_any_rank), L.ptr(handle), C.byref(ptr)))
        return handle.tobytes(), int(ptr.value or 0)

    def peer_connect(self, handles, same_process_ptrs, send_dst_off):
        """handles: list of 64-byte IPC handles in rank order (or None); same_process_ptrs: list of device addresses
        (0: use the handle) or None; send_dst_off[q]: where this rank's rows begin in peer q's ghost area."""
        hb = None if handles is None else np.frombuffer(b''.join(handles), dtype=np.uint8).copy()
        pp = None if same_process_ptrs is None else (C.c_void_p * len(same_process_ptrs))(*[C.c_void_p(int(v) or None) for v in same_process_ptrs])
        off = np.ascontiguousarray(send_dst_off, dtype=np.int64)
        if off.size == 0:
            off = np.zeros(1, dtype=np.int64)
        self._check(self._lib.prcg_peer_connect(self._h, L.ptr(hb), pp, L.ptr(off)))

    def peer_selftest(self, k, rows, slot):
        """One round of the exchange primitives (prcg.h: prcg_peer_selftest): returns (sum of all ranks' slots, ghost area)."""
        rows, slot = L.f64(rows), L.f64(slot)
        assert rows.shape == (self.n, 2) and slot.shape == (5,)
        sums, ghost = np.zeros(5), np.zeros((max(self.n_ghost, 1), 2))
        self._check(self._lib.prcg_peer_selftest(self._h, int(k), L.ptr(rows), L.ptr(slot), L.ptr(sums), L.ptr(ghost)))
        return sums, ghost[:self.n_ghost]

    # -- products (tests / bench) ---------------------------------------------------------
    def matvec(self, x, reps=1):
        """y = A x on the device; returns (y, mean ms per launch)."""
        x = L.f64(x)
        assert x.shape == (self.n,)
        y = np.empty(self.n)
        ms = C.c_double(0.0)
        self._check(self._lib.prcg_spmv(self._h, L.ptr(x), L.ptr(y), int(reps), C.byref(ms)))
        return y, ms.value

    def matvec_ext(self, x_ext):
        """y = A_local [x_own ; x_ghost] with the ghost entries supplied by the caller (no halo
        exchange, no communicator): one rank's share of a row-block product."""
        x_ext = L.f64(x_ext)
        assert x_ext.shape == (self.n + self.n_ghost,)
        y = np.empty(self.n)
        self._check(self._lib.prcg_spmv_ext(self._h, L.ptr(x_ext), L.ptr(y)))
        return y

    def matmat2(self, RS, reps=1):
        """[w u] = A [r s] for an (n,2) array; returns ((n,2) array, mean ms per launch)."""
        RS = L.f64(RS)
        assert RS.shape == (self.n, 2)
        WU = np.empty((self.n, 2))
        ms = C.c_double(0.0)
        self._check(self._lib.prcg_spmm2(self._h, L.ptr(RS), L.ptr(WU), int(reps), C.byref(ms)))
        return WU, ms.value

    def matmat4(self, X, reps=1):
        """[y0 y1 y2 y3] = A [x0 x1 x2 x3] for an (n,4) array, on the route a four-RHS session takes (prcg.h: prcg_spmm4): one
        launch on sliced-row operators, else two two-vector launches; returns ((n,4) array, mean ms per product)."""
        X = L.f64(X)
        assert X.shape == (self.n, 4)
        Y = np.empty((self.n, 4))
        ms = C.c_double(0.0)
        self._check(self._lib.prcg_spmm4(self._h, L.ptr(X), L.ptr(Y), int(reps), C.byref(ms)))
        return Y, ms.value

    # -- solver session ------------------------------------------------------------------------
    def begin(self, variant, b, x0, max_iter, x_true=None, inv_diag=None, hist_mask=0, preconditioner=None, block_jacobi=None,
              block_jacobi_var=None, rr_stop=None):
        """rr_stop: None, or a threshold on r.r, finite and >= 0: THIS session then stops by itself on the device, converged or
        broken down, by the rule of prcg.h: prcg_set_stop (pipelined variants on one GPU, unpreconditioned or with inv_diag), or,
        with block_jacobi= / block_jacobi_var=, prcg_set_stop_block_jacobi (pipelined variants on one GPU with point-block Jacobi,
        set or built on the device: the stored-tilde schedule, every launch in its stop form), or, for L.HS without blocks or a
        callback, prcg_set_stop_hs (Hestenes-Stiefel on one GPU, unpreconditioned or with inv_diag); anything else is refused.
        stop() tells where and why.
        inv_diag: Jacobi on the device.  block_jacobi=(bs, inv_blocks): point-block Jacobi on the device, inv_blocks
        the ceil(n/bs) x bs x bs inverses of the diagonal blocks (prcg.h: prcg_set_block_jacobi); inv_blocks None: the blocks
        BUILT ON THE DEVICE from the operator (build_block_jacobi) -- rebuilt only when blocks of that bs built from the
        current values are not in force already (after update_values, after a session that removed or replaced them).
        preconditioner: any
        callable v -> M^-1 v (what the reference's *_pcg functions take); it runs on the host wherever the reference
        calls it (prcg.h: prcg_set_preconditioner).  block_jacobi_var=(block_ptr, inv_blocks): point-block Jacobi with VARIABLE
        block sizes on the device (prcg.h: prcg_set_block_jacobi_var; inv_blocks packed); inv_blocks None: built on the device
        (build_block_jacobi_var), rebuilt only when blocks of that same partition built from the current values are not in
        force already.  At most one of the four; a session without block_jacobi / block_jacobi_var removes the blocks an earlier
        session on this operator set."""
        b, x0 = L.f64(b), L.f64(x0)
        assert b.shape == (self.n,) and x0.shape == (self.n,)
        assert sum(q is not None for q in (inv_diag, preconditioner, block_jacobi, block_jacobi_var)) <= 1
        xt = None if x_true is None else L.f64(x_true)
        dv = None if inv_diag is None else L.f64(inv_diag)
        if preconditioner is not None:
            n = self.n

            def call(_ctx, count, v, out):
                try:
                    res = np.asarray(preconditioner(np.ctypeslib.as_array(v, shape=(count,)).copy()), dtype=np.float64)
                    if res.shape != (count,):
                        return 2
                    np.ctypeslib.as_array(out, shape=(count,))[:] = res
                    return 0
                except Exception:          # noqa: BLE001 -- reported through the C return code
                    import traceback
                    traceback.print_exc()
                    return 1
            self._prec_fn = L.PREC_FN(call)            # keep the trampoline alive for the whole session
            self._check(self._lib.prcg_set_preconditioner(self._h, C.cast(self._prec_fn, C.c_void_p), None))
            self._no_blocks()                           # (it replaces the blocks)
        else:
            self._prec_fn = None
            self._check(self._lib.prcg_set_preconditioner(self._h, None, None))
        self._put_blocks(block_jacobi, block_jacobi_var)
        thr = None if rr_stop is None else np.array([rr_stop], dtype=np.float64)
        blocks = block_jacobi is not None or block_jacobi_var is not None
        # with blocks the block-Jacobi setter; Hestenes-Stiefel without blocks or a callback stops through a setter of its own
        hs = int(variant) == L.HS and not blocks and preconditioner is None
        with self._stop_request('prcg_set_stop_block_jacobi' if blocks else 'prcg_set_stop_hs' if hs else 'prcg_set_stop', thr):
            self._check(self._lib.prcg_solve_begin(self._h, int(variant), L.ptr(b), L.ptr(x0), int(max_iter),
                                                   L.ptr(xt), L.ptr(dv), int(hist_mask)))
        self.max_iter, self.hist_mask = int(max_iter), int(hist_mask)

    _SINGLE_STOPS = ('prcg_set_stop', 'prcg_set_stop_block_jacobi', 'prcg_set_stop_hs')

    @contextlib.contextmanager
    def _stop_request(self, setter, thr):
        """The handle's stop requests around ONE begin (prcg.h: prcg_set_stop, _block_jacobi, _hs, _rhs).  `setter`, the one the
        session needs, gets thr -- None clears what an earlier session set -- and the other setters of single sessions get None
        (prcg_set_stop_rhs has its begin to itself).  Afterwards the handle is restored: a threshold is this session's, so its
        request is cleared and the begins that refuse it are served again; prcg_set_stop's stays, no other begin consults it."""
        single = setter in self._SINGLE_STOPS
        for name in self._SINGLE_STOPS if single else (setter,):
            value = L.ptr(thr if name == setter else None)
            self._check(getattr(self._lib, name)(self._h, *((value,) if single else (2, value))))
        try:
            yield
        finally:
            if thr is not None and setter != 'prcg_set_stop':
                self._check(getattr(self._lib, setter)(self._h, *((None,) if single else (0, None))))

    def _put_blocks(self, block_jacobi, block_jacobi_var):
        """The blocks a session asks for, put in force on the handle (begin, begin_multi_block_jacobi): (bs, inv_blocks) or
        (block_ptr, inv_blocks_packed) are set; inv_blocks None means BUILT on the device, rebuilt only when blocks of that bs /
        partition built from the current values are not in force already; neither: whatever blocks are set are removed."""
        if block_jacobi is not None and block_jacobi[1] is None:
            if self._bj_built is None or self._bj_built != int(block_jacobi[0]):
                self.build_block_jacobi(int(block_jacobi[0]))
        elif block_jacobi is not None:
            self.set_block_jacobi(block_jacobi[0], block_jacobi[1])
        elif block_jacobi_var is not None and block_jacobi_var[1] is None:
            ptr = self._partition(block_jacobi_var[0], 'block_jacobi_var')
            if self._bjv_built is None or not np.array_equal(self._bjv_built, ptr):
                self.build_block_jacobi_var(ptr)
        elif block_jacobi_var is not None:
            self.set_block_jacobi_var(block_jacobi_var[0], block_jacobi_var[1])
        else:
            self.set_block_jacobi(0, None)

    def clear_preconditioners(self):
        """Remove a host-callback or block-Jacobi preconditioner an earlier session set on this handle."""
        self._prec_fn = None
        self._check(self._lib.prcg_set_preconditioner(self._h, None, None))
        self.set_block_jacobi(0, None)

    def begin_multi(self, variant, B, X0, max_iter, inv_diag=None, hist_mask=0):
        """Two or four right-hand sides in ONE session (prcg.h: prcg_solve_begin_multi): B, X0 of shape (2, n) or (4, n), both
        the same, row j = right-hand side / start vector of system j.  Every iteration streams the operator once for all systems
        (four systems: in one launch on sliced-row operators, see schedule()['spmm4']).
        variant: L.HS (hs_cg / hs_pcg), L.PR (pr_cg / pr_pcg) or L.M (m_cg / m_pcg); inv_diag: Jacobi on the device (the same
        diagonal for both); hist_mask: 0 or updated_residual_2_norm.
        iterate / sync / k serve the session as they are; state is read per column: get_vector(name, rhs=j), get_scalars(k, rhs=j),
        get_coefficients(k, rhs=j), history(rhs=j)."""
        B = _pair_of_vectors('B', B, self.n)
        X0 = _pair_of_vectors('X0', X0, self.n, nrhs=B.shape[0])
        dv = _diagonal('begin_multi', inv_diag, self.n)
        self._check(self._lib.prcg_solve_begin_multi(self._h, int(variant), len(B), _row_pointers(B), _row_pointers(X0), int(max_iter),
                                                     L.ptr(dv), int(hist_mask)))
        self.max_iter, self.hist_mask = int(max_iter), int(hist_mask)

    def begin_multi_block_jacobi(self, variant, B, X0, max_iter, block_jacobi=None, block_jacobi_var=None, hist_mask=0):
        """Two or four right-hand sides in ONE session preconditioned by point-block Jacobi on the device (prcg.h:
        prcg_solve_begin_multi_block_jacobi): B, X0 of shape (2, n) or (4, n).  variant: L.HS (hs_pcg), L.PR (pr_pcg) or L.M (m_pcg).
        Exactly one of block_jacobi=(bs, inv_blocks) / (bs, None) and block_jacobi_var=(block_ptr, inv_blocks_packed) /
        (block_ptr, None), with the conventions of begin: None means built on the device from the operator's current values,
        rebuilt only if such blocks are not in force already.  hist_mask: 0 or updated_residual_2_norm.
        Every iteration streams the operator once for all systems and reads every block once per pair of systems.  iterate /
        sync / k serve the session as they are; state is read per column: get_vector(name, rhs=j) (x, r, p, s, rt; PR / M: st),
        get_scalars(k, rhs=j), get_coefficients(k, rhs=j), history(rhs=j).  The blocks stay on the handle afterwards."""
        B = _pair_of_vectors('B', B, self.n)
        X0 = _pair_of_vectors('X0', X0, self.n, nrhs=B.shape[0])
        if (block_jacobi is None) == (block_jacobi_var is None):
            raise ValueError('begin_multi_block_jacobi: exactly one of block_jacobi= and block_jacobi_var= must be given '
                             '(without blocks the session is begin_multi)')
        self._prec_fn = None
        self._check(self._lib.prcg_set_preconditioner(self._h, None, None))
        self._put_blocks(block_jacobi, block_jacobi_var)
        self._check(self._lib.prcg_solve_begin_multi_block_jacobi(self._h, int(variant), len(B), _row_pointers(B), _row_pointers(X0),
                                                                  int(max_iter), int(hist_mask)))
        self.max_iter, self.hist_mask = int(max_iter), int(hist_mask)

    def begin_multi_pipe(self, variant, B, X0, max_iter, inv_diag=None, hist_mask=0, rr_stop=None):
        """Two right-hand sides in ONE pipelined session (prcg.h: prcg_solve_begin_multi_pipe): B, X0 of shape (2, n), row j =
        right-hand side / start vector of system j.  Every iteration streams the operator once for both systems: the pipelined
        iteration's [w u] = A [r s] of both columns is one product of four vectors (one launch on sliced-row operators, see
        schedule()['spmm4']).
        variant: L.PIPE_PR (pipe_pr_cg / pipe_pr_pcg) or L.PIPE_PR_M (pipe_pr_m_cg / pipe_pr_m_pcg); inv_diag: Jacobi on the device
        (the same diagonal for both); hist_mask: 0 or updated_residual_2_norm.  begin_multi keeps refusing the pipelined variants.
        Which to prefer: this session where the operator dominates an iteration's traffic (assembled FEM matrices, sliced rows);
        on band and stencil operators two single sessions, each ONE launch per iteration, may well be faster -- see
        profiles/multi_rhs_pipe.md for what was measured.
        iterate / sync / k serve the session as they are; state is read per column: get_vector(name, rhs=j) (x, r, p, s, w, u; with
        Jacobi rt, st), get_scalars(k, rhs=j), get_coefficients(k, rhs=j), history(rhs=j).
        rr_stop: None, or two thresholds on r.r, one per column, each finite and >= 0: THIS session then stops each column by itself
        on the device at its own threshold, converged or broken down, by the rule of prcg.h: prcg_set_stop_rhs -- the stopped
        column keeps the state of its stop iteration, the other runs on with the bits it has without thresholds; stops_rhs()
        tells where and why."""
        thr = None if rr_stop is None else batch_thresholds('rr_stop', np.asarray(rr_stop, dtype=np.float64).reshape(-1), 2)
        B = L.f64(B)
        if B.shape != (2, self.n):
            raise ValueError(f'begin_multi_pipe: B must have shape (2, {self.n}) -- the pipelined session serves exactly two right-hand '
                             f'sides of the operator\'s size -- got {tuple(B.shape)}')
        X0 = L.f64(X0)
        if X0.shape != (2, self.n):
            raise ValueError(f'begin_multi_pipe: X0 must have shape (2, {self.n}), the same as B, got {tuple(X0.shape)}')
        dv = _diagonal('begin_multi_pipe', inv_diag, self.n)
        with self._stop_request('prcg_set_stop_rhs', thr):
            self._begin_multi_pipe(variant, B, X0, max_iter, dv, hist_mask)

    def _begin_multi_pipe(self, variant, B, X0, max_iter, dv, hist_mask):
        self._check(self._lib.prcg_solve_begin_multi_pipe(self._h, int(variant), 2, _row_pointers(B), _row_pointers(X0), int(max_iter),
                                                          L.ptr(dv), int(hist_mask)))
        self.max_iter, self.hist_mask = int(max_iter), int(hist_mask)

    def set_replace_hook(self, fn):
        """Ghysels-Vanroose residual replacement (prcg.h: prcg_set_replace_hook): fn(k) -> truthy replaces w by A r in
        iteration k; None removes the hook.  Set before begin()."""
        if fn is None:
            self._replace_fn = None
            self._check(self._lib.prcg_set_replace_hook(self._h, None, None))
            return

        def call(_ctx, k):
            try:
                return 1 if fn(int(k)) else 0
            except Exception:          # noqa: BLE001 -- a failing predicate does not replace; the traceback is shown
                import traceback
                traceback.print_exc()
                return 0
        self._replace_fn = L.REPLACE_FN(call)          # keep the trampoline alive
        self._check(self._lib.prcg_set_replace_hook(self._h, C.cast(self._replace_fn, C.c_void_p), None))

    def iterate(self, iters):
        self._check(self._lib.prcg_iterate(self._h, int(iters)))

    def sync(self):
        self._check(self._lib.prcg_sync(self._h))

    @property
    def k(self):
        return self._lib.prcg_iteration(self._h)

    def stop(self):
        """(k_stop, status) of the open single session: the iteration it stopped at and why (1 converged, 2 breakdown); (-1, 0)
        while it runs, and for a session begun without rr_stop.  Synchronises."""
        k_stop, status = C.c_int32(-1), C.c_int32(0)
        self._check(self._lib.prcg_get_stop(self._h, C.byref(k_stop), C.byref(status)))
        return int(k_stop.value), int(status.value)

    def stops_rhs(self):
        """[(k_stop, status), (k_stop, status)] of the open two-RHS session's columns: the iteration a column stopped at and why
        (1 converged, 2 breakdown); (-1, 0) for a column that still runs, and for both in a session begun without rr_stop (four
        entries in a four-RHS session).  Synchronises."""
        k_stop, status = np.full(4, -1, dtype=np.int32), np.zeros(4, dtype=np.int32)
        self._check(self._lib.prcg_get_stops_rhs(self._h, L.ptr(k_stop), L.ptr(status)))
        nrhs = 4 if self.schedule()['rhs4'] else 2
        return [(int(k_stop[c]), int(status[c])) for c in range(nrhs)]

    def schedule(self):
        """Flags of the schedule the current session runs (prcg.h PRCG_SCHED_*)."""
        s = self._lib.prcg_schedule(self._h)
        return {'fused': bool(s & 1), 'small': bool(s & 2), 'comm': bool(s & 4), 'gather': bool(s & 8),
                'dual_comm': bool(s & 16), 'value_dict': bool(s & 32),
                'col_bytes': 0 if s & 65536 else (1 if s & 64 else (2 if s & 128 else 4)), 'tile_steps': (s >> 8) & 15,
                'pattern': bool(s & 65536), 'window': bool(s & 4096), 'fused_comm': bool(s & 8192), 'peer': bool(s & 16384), 'sliced_rows': bool(s & 32768),
                'stream_stores': bool(s & 131072), 'sorted_windows': bool(s & 262144), 'nt_loads': bool(s & 524288), 'window_codes': bool(s & 2097152),
                'block_jacobi': bool(s & 4194304), 'xp_deferred': bool(s & 8388608), 'rhs2': bool(s & 16777216),
                'rhs4': bool(s & 33554432), 'spmm4': bool(s & 67108864), 'rhs2_pipe': bool(s & 134217728),
                'block_jacobi_var': bool(s & 268435456)}

    def layout(self):
        """Diagnostic (prcg_test.h: prcg_debug_layout): what the summation order of a tile launch's inner products depends
        on -- tile rows in table order, and 'grid' / 'waves_per_block' of the session's LAST launch that left inner-product
        partials (any schedule's iteration launch, or the start-up products right after begin(); never a recorder's;
        grid 0: none yet).  A session without a communicator leaves the partials of an iteration from ONE tile launch; with one,
        the two-kernel schedules run a product with a dot epilogue as two launches -- 'grid' / 'waves_per_block' are then the
        boundary launch's (tiles[interior_tiles:]) and 'interior_grid' / 'interior_waves_per_block' the interior launch's
        (tiles[:interior_tiles], its partial rows first); both 0 when the last such launch ran over all the tiles.
        'sliced': the operator runs on sliced rows; 'slice_rows' (prcg_debug_slice_rows): then the row of every lane of
        every slice in launch order (interior slices first), shape (slices, 64), -1 for an idle lane -- else shape (0, 64);
        'interior_slices' (prcg_debug_interior_slices): slice_rows[:interior_slices] hold no row with a ghost column and are what
        the interior launch of such a product runs on sliced rows ('interior_tiles' counts tiles, whatever runs); else 0."""
        need = -int(self._lib.prcg_debug_layout(self._h, L.ptr(np.zeros(1, dtype=np.int64)), 0))
        out = np.zeros(max(need, 10), dtype=np.int64)
        got = int(self._lib.prcg_debug_layout(self._h, L.ptr(out), out.size))
        if got < 10:
            raise RuntimeError('prcg_debug_layout failed')
        need = -int(self._lib.prcg_debug_slice_rows(self._h, None, 0))
        if need < 0 or need % 64:                      # (-1: an error; -needed is a multiple of 64)
            raise RuntimeError('prcg_debug_slice_rows failed')
        rows = np.zeros(need, dtype=np.int32)
        if need and int(self._lib.prcg_debug_slice_rows(self._h, L.ptr(rows), rows.size)) != need:
            raise RuntimeError('prcg_debug_slice_rows failed')
        nst_int = int(self._lib.prcg_debug_interior_slices(self._h))
        if nst_int < 0 or 64 * nst_int > need:
            raise RuntimeError('prcg_debug_interior_slices failed')
        return {'window': bool(out[0]), 'geometry': int(out[1]), 'rows_per_tile': int(out[2]), 'tiles': out[10:got].reshape(-1, 2).copy(),
                'grid': int(out[4]), 'waves_per_block': int(out[5]), 'interior_tiles': int(out[6]), 'sweep_waves': int(out[7]) >> 8,
                'interior_grid': int(out[8]), 'interior_waves_per_block': int(out[9]),
                'sliced': need > 0, 'slice_rows': rows.reshape(-1, 64), 'interior_slices': nst_int}

    def operator_bytes(self):
        """Bytes of the operator as the device streams it (prcg.h: prcg_operator_bytes)."""
        return int(self._lib.prcg_operator_bytes(self._h))

    def set_iteration(self, k):
        self._check(self._lib.prcg_set_iteration(self._h, int(k)))

    def get_vector(self, name, *, rhs=None):
        """rhs=j: column j of a two- or four-RHS session (begin_multi): x, r, p, s; with Jacobi rt, and in an L.PR / L.M session st.
        In a pipelined two-RHS session (begin_multi_pipe) also w and u, and with Jacobi rt and st.  In a block-Jacobi session
        (begin_multi_block_jacobi) x, r, p, s, rt, and for L.PR / L.M st."""
        out = np.empty(self.n)
        if rhs is None:
            self._check(self._lib.prcg_get_vector(self._h, L.VEC[name], L.ptr(out)))
        else:
            self._check(self._lib.prcg_get_vector_rhs(self._h, L.VEC[name], int(rhs), L.ptr(out)))
        return out

    def set_vector(self, name, v):
        v = L.f64(v)
        assert v.shape == (self.n,)
        self._check(self._lib.prcg_set_vector(self._h, L.VEC[name], L.ptr(v)))

    def get_scalars(self, k, *, rhs=None):
        out = np.empty(L.NUM_SCALARS)
        if rhs is None:
            self._check(self._lib.prcg_get_scalars(self._h, int(k), L.ptr(out)))
        else:
            self._check(self._lib.prcg_get_scalars_rhs(self._h, int(k), int(rhs), L.ptr(out)))
        return out

    def set_scalars(self, k, values):
        v = L.f64(values)
        assert v.shape == (L.NUM_SCALARS,)
        self._check(self._lib.prcg_set_scalars(self._h, int(k), L.ptr(v)))

    def get_coefficients(self, k, *, rhs=None):
        out = np.empty(3)
        if rhs is None:
            self._check(self._lib.prcg_get_coefficients(self._h, int(k), L.ptr(out)))
        else:
            self._check(self._lib.prcg_get_coefficients_rhs(self._h, int(k), int(rhs), L.ptr(out)))
        return out

    def history(self, *, rhs=None):
        """dict recorder-name -> array(max_iter) for the recorders of this session (rhs=j: of column j of a two-RHS session)."""
        names = [q for q, bit in sorted(L.HIST_BITS.items(), key=lambda kv: kv[1]) if self.hist_mask & bit]
        if not names:
            return {}
        buf = np.zeros((len(names), self.max_iter))
        if rhs is None:
            self._check(self._lib.prcg_get_history(self._h, L.ptr(buf)))
        else:
            self._check(self._lib.prcg_get_history_rhs(self._h, int(rhs), L.ptr(buf)))
        return {q: buf[i].copy() for i, q in enumerate(names)}

    def set_profiling(self, stride):
        self._check(self._lib.prcg_set_profiling(self._h, int(stride)))

    def stream_ceiling(self, n_pairs, mode, reps=20):
        """GB/s the memory system delivers for a byte mix over arrays of n_pairs 16-byte entries (prcg_test.h:
        prcg_stream_ceiling): mode 0 pure read, 1 = 2 x 16 B in + 2 x 16 B out per row (the one-launch iteration's vector
        traffic) with plain stores, 2 with nontemporal stores, 3 pure read in contiguous 4 KB chunks per wave, nontemporal."""
        g = C.c_double()
        self._check(self._lib.prcg_stream_ceiling(self._h, int(n_pairs), int(mode), int(reps), C.byref(g)))
        return float(g.value)

    def mix_ceiling(self, n_rows, stream_kb_per_64_rows, reps=10):
        """GB/s the memory system delivers for the byte mix of a one-launch iteration that streams that many KB of operator per 64
        rows beside the rows' 64 B of vector traffic (prcg_test.h: prcg_mix_ceiling)."""
        g = C.c_double()
        self._check(self._lib.prcg_mix_ceiling(self._h, int(n_rows), int(stream_kb_per_64_rows), int(reps), C.byref(g)))
        return float(g.value)

    def timings(self):
        t = L.Timings()
        self._check(self._lib.prcg_get_timings(self._h, C.byref(t)))
        return t.as_dict()

    def solve(self, variant, b, x0, max_iter, x_true=None, inv_diag=None, hist_mask=0):
        """One C call: begin + (max_iter-1) iterations + histories + x (prcg_solve)."""
        b, x0 = L.f64(b), L.f64(x0)
        xt = None if x_true is None else L.f64(x_true)
        dv = None if inv_diag is None else L.f64(inv_diag)
        nh = bin(hist_mask).count('1')
        hist = np.zeros((max(nh, 1), max_iter))
        x = np.empty(self.n)
        t = L.Timings()
        self._check(self._lib.prcg_solve(self._h, int(variant), L.ptr(b), L.ptr(x0), int(max_iter), L.ptr(xt),
                                         L.ptr(dv), int(hist_mask), L.ptr(hist) if nh else None, L.ptr(x),
                                         C.byref(t)))
        self.max_iter, self.hist_mask = int(max_iter), int(hist_mask)
        names = [q for q, bit in sorted(L.HIST_BITS.items(), key=lambda kv: kv[1]) if hist_mask & bit]
        return x, {q: hist[i].copy() for i, q in enumerate(names)}, t.as_dict()


def batch_matrices(As, n_sys=None):
    """(matrices, mat_of) of a batch from what the caller passes as `As`: ONE matrix (every one of the n_sys systems uses it) or a
    sequence of matrices, one per system -- entries that are the same object become one matrix of the batch (one upload).
    Pure host work; ValueError names what is wrong."""
    if hasattr(As, 'indptr'):
        if n_sys is None:
            raise ValueError('one matrix for every system needs the number of systems')
        return [As], [0] * int(n_sys)
    As = list(As)
    if n_sys is not None and len(As) != n_sys:
        raise ValueError(f'As must be one matrix or a sequence of {n_sys} matrices, one per right-hand side -- got {len(As)}')
    matrices, mat_of, seen = [], [], {}
    for A in As:
        if not hasattr(A, 'indptr'):
            raise TypeError('every entry of As must be a scipy.sparse CSR matrix/array')
        if id(A) not in seen:
            seen[id(A)] = len(matrices)
            matrices.append(A)
        mat_of.append(seen[id(A)])
    return matrices, mat_of


def batch_vectors(name, V, sizes):
    """The systems' vectors concatenated in system order (1-D float64) from a list of vectors or, when all sizes agree, one 2-D
    array (n_sys, n); ValueError names the expected shape."""
    n_sys = len(sizes)
    if isinstance(V, np.ndarray) and V.ndim == 2:
        if len(set(sizes)) != 1:
            raise ValueError(f'{name} is one 2-D array of shape {tuple(V.shape)} but the systems have different sizes: pass a list of '
                             f'{n_sys} vectors, {name}[s] of shape (n_s,)')
        if V.shape != (n_sys, sizes[0]):
            raise ValueError(f'{name} must have shape ({n_sys}, {sizes[0]}) -- one row per system -- got {tuple(V.shape)}')
        return L.f64(V).reshape(-1)
    V = list(V)
    if len(V) != n_sys:
        raise ValueError(f'{name} must hold {n_sys} vectors, one per system -- got {len(V)}')
    out = np.empty(int(sum(sizes)))
    at = 0
    for s, (v, n) in enumerate(zip(V, sizes)):
        v = np.asarray(v, dtype=np.float64)
        if v.shape != (n,):
            raise ValueError(f'{name}[{s}] must have shape ({n},), the size of system {s} -- got {tuple(v.shape)}')
        out[at:at + n] = v
        at += n
    return out


def batch_blocks(name, blocks, sizes):
    """(nblk_off, block_ptr, inv_blocks) as prcg_batch_begin_block_jacobi takes them (prcg.h) from one (block_ptr, inv_blocks)
    per system: block_ptr the system's partition (nb + 1 entries, zero-based, from 0 to n_s), inv_blocks its packed inverses
    (block k as m_k x m_k row-major; any shape with sum of m_k^2 entries).  Pure host work; ValueError names the system and what
    is wrong with its shapes -- the partition's values are the library's to refuse."""
    blocks = list(blocks)
    if len(blocks) != len(sizes):
        raise ValueError(f'{name} must hold {len(sizes)} pairs (block_ptr, inv_blocks), one per system -- got {len(blocks)}')
    ptrs, invs = [], []
    for s, pair in enumerate(blocks):
        try:
            ptr, inv = pair
        except (TypeError, ValueError):
            raise ValueError(f'{name}[{s}] must be a pair (block_ptr, inv_blocks)') from None
        ptr = np.ascontiguousarray(ptr, dtype=np.int64)
        inv = np.ascontiguousarray(inv, dtype=np.float64).reshape(-1)
        if ptr.ndim != 1 or ptr.size < 1:
            raise ValueError(f'{name}[{s}]: block_ptr must be a one-dimensional array of nb + 1 entries, got shape {ptr.shape}')
        need = int(np.sum(np.diff(ptr) ** 2))
        if inv.size != need:
            raise ValueError(f'{name}[{s}]: inv_blocks holds {inv.size} entries, the partition\'s blocks have {need} (packed: block k is '
                             'm_k x m_k, no padding)')
        ptrs.append(ptr)
        invs.append(inv)
    nblk_off = np.concatenate([[0], np.cumsum([p.size - 1 for p in ptrs])]).astype(np.int64)
    return nblk_off, np.concatenate(ptrs), np.concatenate(invs) if invs else np.empty(0)


def batch_thresholds(name, v, n_sys):
    """One finite value >= 0 per system (1-D float64) from a scalar -- every system's -- or a sequence of n_sys; ValueError names
    the count or the first system whose value is NaN, infinite or negative.  Pure host work."""
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 0:
        a = np.full(n_sys, float(a))
    if a.shape != (n_sys,):
        raise ValueError(f'{name} must be one value or {n_sys} values, one per system -- got shape {tuple(a.shape)}')
    bad = np.flatnonzero(~(np.isfinite(a) & (a >= 0)))
    if bad.size:
        raise ValueError(f'{name}[{bad[0]}] = {a[bad[0]]}: the value of system {bad[0]} must be finite and >= 0')
    return np.ascontiguousarray(a)


class DeviceBatch:
    """A batch of small independent systems A_s x_s = b_s solved in ONE launch, one workgroup per system (prcg.h:
    prcg_batch_create): what a Python loop over ``DeviceCSR(A).begin(...); iterate(...)`` computes for matrices that fit the
    one-workgroup solver, without a handle, a planning pass and a launch per system.

    ``matrices``: a sequence of scipy.sparse CSR matrices; ``mat_of[s]``: the matrix of system s (default: system s uses
    matrix s).  Systems that share a matrix share its upload.  Every system must fit the one-workgroup solver (n <= 4096, the
    matrix in registers or LDS): anything else is refused, a batch has no other schedule.
    """

    def __init__(self, matrices, mat_of=None, device=0):
        if hasattr(matrices, 'indptr'):
            matrices = [matrices]
        mats = []
        for A in matrices:
            if not hasattr(A, 'indptr'):
                raise TypeError('every matrix must be a scipy.sparse CSR matrix/array')
            if A.format != 'csr':
                A = A.tocsr()
            if A.dtype != np.float64:
                raise TypeError(f'fp64 only (got {A.dtype}); the reference works in double precision')
            if A.shape[0] != A.shape[1]:
                raise ValueError(f'a system of a batch is square, got a matrix of shape {A.shape}')
            mats.append(A)
        if not mats:
            raise ValueError('a batch holds at least one matrix')
        mat_of = np.arange(len(mats), dtype=np.int32) if mat_of is None else np.ascontiguousarray(mat_of, dtype=np.int32)
        if mat_of.ndim != 1:
            raise ValueError(f'mat_of must be one-dimensional, got shape {mat_of.shape}')
        rows_off = np.concatenate([[0], np.cumsum([A.shape[0] for A in mats])]).astype(np.int64)
        nnz_off = np.concatenate([[0], np.cumsum([A.nnz for A in mats])]).astype(np.int64)
        indptr = np.concatenate([np.asarray(A.indptr, dtype=np.int32) for A in mats])
        indices = np.ascontiguousarray(np.concatenate([A.indices for A in mats]), dtype=np.int32)
        data = np.ascontiguousarray(np.concatenate([A.data for A in mats]), dtype=np.float64)
        self._lib = L.lib()
        self._h, self._b = C.c_void_p(), C.c_void_p()
        self.device = int(device)
        rc = self._lib.prcg_create(C.byref(self._h), int(device))
        if rc != L.OK:
            msg = self._lib.prcg_last_error(None)
            self._h = C.c_void_p()
            raise L.PrcgError(rc, msg.decode() if msg else '?')
        try:
            self._check(self._lib.prcg_batch_create(self._h, len(mats), L.ptr(rows_off), L.ptr(nnz_off), L.ptr(indptr), L.ptr(indices),
                                                    L.ptr(data), int(mat_of.size), L.ptr(mat_of), C.byref(self._b)))
        except Exception:
            self.close()
            raise
        self.n_sys = int(mat_of.size)
        self.sizes = [int(mats[m].shape[0]) for m in mat_of]
        self.max_iter, self.hist_mask = 0, 0

    def _check(self, rc):
        L.check(self._h, rc)

    def close(self):
        if getattr(self, '_b', None) is not None and self._b.value:
            self._lib.prcg_batch_destroy(self._b)
            self._b = C.c_void_p()
        if getattr(self, '_h', None) is not None and self._h.value:
            self._lib.prcg_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def begin(self, variant, B, X0, max_iter, hist_mask=0, inv_diag=None, rr_stop=None, block_jacobi=None):
        """variant: L.PIPE_PR, L.PIPE_PR_M or L.HS.  B, X0: a list of vectors, one per system, or one 2-D array (n_sys, n) when
        all sizes agree.  hist_mask: 0 or L.HIST_UPDATED_RESIDUAL_2_NORM.  inv_diag: None, or -- in the form of B -- every
        system's reciprocal diagonal: the session is then preconditioned by that scaling inside the one-workgroup solver
        (prcg.h: prcg_batch_begin_jacobi), and a pipelined one also serves get_vector('rt' / 'st', s).  rr_stop: None, or a
        threshold on r.r -- one per system, or a scalar for all --: every system of THIS session then stops by itself, converged
        or broken down, by the rule of prcg.h: prcg_batch_set_stop; stops() tells where and why.  block_jacobi: None, or one
        pair (block_ptr, inv_blocks) per system -- its partition (every size in 1..8) and the packed inverses of its diagonal
        blocks, what VarBlockJacobi carries --: the session is preconditioned by point-block Jacobi inside the one-workgroup
        solver (prcg.h: prcg_batch_begin_block_jacobi); state and accessors as with inv_diag, with which it cannot be combined."""
        if inv_diag is not None and block_jacobi is not None:
            raise ValueError('inv_diag and block_jacobi are mutually exclusive: a session has one preconditioner')
        b, x0 = batch_vectors('B', B, self.sizes), batch_vectors('X0', X0, self.sizes)
        blocks = None if block_jacobi is None else batch_blocks('block_jacobi', block_jacobi, self.sizes)
        d = None if inv_diag is None else batch_vectors('inv_diag', inv_diag, self.sizes)
        thr = None if rr_stop is None else batch_thresholds('rr_stop', rr_stop, self.n_sys)
        self._check(self._lib.prcg_batch_set_stop(self._b, L.ptr(thr)))      # (None clears what an earlier session set)
        if blocks is not None:
            self._check(self._lib.prcg_batch_begin_block_jacobi(self._b, int(variant), L.ptr(b), L.ptr(x0), L.ptr(blocks[0]), L.ptr(blocks[1]),
                                                                L.ptr(blocks[2]), int(max_iter), int(hist_mask)))
        elif inv_diag is None:
            self._check(self._lib.prcg_batch_begin(self._b, int(variant), L.ptr(b), L.ptr(x0), int(max_iter), int(hist_mask)))
        else:
            self._check(self._lib.prcg_batch_begin_jacobi(self._b, int(variant), L.ptr(b), L.ptr(x0), L.ptr(d), int(max_iter), int(hist_mask)))
        self.max_iter, self.hist_mask = int(max_iter), int(hist_mask)

    def iterate(self, iters):
        self._check(self._lib.prcg_batch_iterate(self._b, int(iters)))

    def sync(self):
        self._check(self._lib.prcg_batch_sync(self._b))

    @property
    def k(self):
        return self._lib.prcg_batch_iteration(self._b)

    def stops(self):
        """(k_stop, status), int32 arrays of n_sys: the iteration every system stopped at and why (1 converged, 2 breakdown); -1
        and 0 for a system that still runs, and for every system of a session begun without rr_stop.  Synchronises."""
        k_stop, status = np.empty(self.n_sys, dtype=np.int32), np.empty(self.n_sys, dtype=np.int32)
        self._check(self._lib.prcg_batch_get_stops(self._b, L.ptr(k_stop), L.ptr(status)))
        return k_stop, status

    def get_vector(self, name, s):
        out = np.empty(self.sizes[s])
        self._check(self._lib.prcg_batch_get_vector(self._b, L.VEC[name], int(s), L.ptr(out)))
        return out

    def solutions(self):
        """every system's x, concatenated in system order (one copy from the device)"""
        out = np.empty(int(sum(self.sizes)))
        self._check(self._lib.prcg_batch_get_solutions(self._b, L.ptr(out)))
        return out

    def get_scalars(self, k, s):
        out = np.empty(L.NUM_SCALARS)
        self._check(self._lib.prcg_batch_get_scalars(self._b, int(k), int(s), L.ptr(out)))
        return out

    def get_coefficients(self, k, s):
        out = np.empty(3)
        self._check(self._lib.prcg_batch_get_coefficients(self._b, int(k), int(s), L.ptr(out)))
        return out

    def history(self, s):
        """dict recorder-name -> array(max_iter) of system s ({} when hist_mask was 0)"""
        if not self.hist_mask & L.HIST_UPDATED_RESIDUAL_2_NORM:
            return {}
        buf = np.zeros(self.max_iter)
        self._check(self._lib.prcg_batch_get_history(self._b, int(s), L.ptr(buf)))
        return {'updated_residual_2_norm': buf}


def multi_rhs_shape_error(name, shape, n, nrhs=None):
    """None if `shape` is (2, n) or (4, n) -- (nrhs, n) when nrhs is given -- else the text of the ValueError."""
    if len(shape) == 2 and shape[1] == n and shape[0] in ((2, 4) if nrhs is None else (nrhs,)):
        return None
    if nrhs in (2, 4):
        return (f'{name} must have shape (2, {n}) or (4, {n}), the same as B -- here ({nrhs}, {n}) -- got {tuple(shape)}')
    return (f'{name} must have shape (2, {n}) or (4, {n}) -- two or four right-hand sides of the operator\'s size -- '
            f'got {tuple(shape)}')


def _pair_of_vectors(name, V, n, nrhs=None):
    """(2, n) or (4, n) C-contiguous float64 ((nrhs, n) when nrhs is given), or ValueError: the multi-RHS session takes two
    or four systems of the operator's size."""
    V = L.f64(V)
    err = multi_rhs_shape_error(name, V.shape, n, nrhs)
    if err:
        raise ValueError(err)
    return V


def _row_pointers(V):
    """the C array of row pointers a multi-RHS entry takes; V is C-contiguous float64 and outlives the call"""
    return (C.c_void_p * len(V))(*[V[j].ctypes.data for j in range(len(V))])


def _diagonal(who, inv_diag, n):
    """inv_diag of a multi-RHS session as float64 of shape (n,), None as None, or ValueError in the name of the method"""
    dv = None if inv_diag is None else L.f64(inv_diag)
    if dv is not None and dv.shape != (n,):
        raise ValueError(f'{who}: inv_diag must have shape ({n},), got {dv.shape}')
    return dv


def plan_tiles(indptr, row_class=None, cap_nnz=None, cap_rows=None):
    """Host-only view of the CSR-adaptive tiling (no GPU needed): returns
    (tiles[(row_begin,row_end)], n_class0)."""
    lib = L.lib()
    if cap_nnz is None or cap_rows is None:
        a, b = C.c_int(0), C.c_int(0)
        lib.prcg_tile_caps(C.byref(a), C.byref(b))
        cap_nnz = cap_nnz or a.value
        cap_rows = cap_rows or b.value
    indptr = np.ascontiguousarray(indptr, dtype=np.int32)
    n = len(indptr) - 1
    rc = None if row_class is None else np.ascontiguousarray(row_class, dtype=np.uint8)
    cap = n + 1
    out = np.zeros((cap, 2), dtype=np.int32)
    n0 = C.c_int64(0)
    got = lib.prcg_plan_tiles(n, L.ptr(indptr), L.ptr(rc), int(cap_nnz), int(cap_rows), L.ptr(out), cap,
                              C.byref(n0))
    if got < 0:
        raise RuntimeError('prcg_plan_tiles failed')
    return out[:got].copy(), int(n0.value)


PLAN_OPERATOR_FIELDS = ('family', 'win_geom', 'rows_per_tile', 'pattern', 'sweep_waves', 'value_dict', 'value_dict_boundary',
                        'col_bytes', 'col_bytes_boundary', 'tile_steps', 'tiles_interior', 'tiles_boundary', 'image_period',
                        'operator_bytes', 'hash_index', 'hash_value_index', 'hash_dictionary', 'hash_tiles')


def plan_values_route(A, knobs=None):
    """Host-only: the route DeviceCSR(A, knobs=knobs).update_values would take (prcg_test.h: prcg_plan_values_route),
    'in_place' or 'replanned'."""
    lib = L.lib()
    A = A.tocsr()
    n_rows, n_cols = A.shape
    indptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
    indices = np.ascontiguousarray(A.indices, dtype=np.int32)
    data = np.ascontiguousarray(A.data, dtype=np.float64)
    items = [(str(k).encode(), str(v).encode()) for k, v in (knobs or {}).items()]
    keys = (C.c_char_p * max(len(items), 1))(*[k for k, _ in items])
    values = (C.c_char_p * max(len(items), 1))(*[v for _, v in items])
    route = int(lib.prcg_plan_values_route(int(n_rows), int(n_cols - n_rows), int(A.nnz), L.ptr(indptr), L.ptr(indices), L.ptr(data),
                                           keys, values, len(items)))
    if route not in (0, 1):
        raise RuntimeError(f'prcg_plan_values_route failed ({route})')
    return ('in_place', 'replanned')[route]


def plan_operator(A, knobs=None):
    """Host-only view of what prcg_set_csr decides for the row block ``A`` under the PRCG_* ``knobs`` (no handle, no GPU):
    a dict of PLAN_OPERATOR_FIELDS -- family 0 = CSR-adaptive tiles, 1 = window tiles, 2 = sliced rows; the four hashes
    are 64-bit FNV-1a sums (as unsigned integers) of the arrays an upload would copy (include/prcg_test.h)."""
    lib = L.lib()
    A = A.tocsr()
    n_rows, n_cols = A.shape
    indptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
    indices = np.ascontiguousarray(A.indices, dtype=np.int32)
    data = np.ascontiguousarray(A.data, dtype=np.float64)
    items = [(str(k).encode(), str(v).encode()) for k, v in (knobs or {}).items()]
    keys = (C.c_char_p * max(len(items), 1))(*[k for k, _ in items])
    values = (C.c_char_p * max(len(items), 1))(*[v for _, v in items])
    out = np.zeros(len(PLAN_OPERATOR_FIELDS), dtype=np.int64)
    got = lib.prcg_plan_operator(int(n_rows), int(n_cols - n_rows), int(A.nnz), L.ptr(indptr), L.ptr(indices), L.ptr(data),
                                 keys, values, len(items), L.ptr(out), out.size)
    if got != out.size:
        raise RuntimeError(f'prcg_plan_operator failed ({got})')
    res = {f: int(v) for f, v in zip(PLAN_OPERATOR_FIELDS, out)}
    for f in PLAN_OPERATOR_FIELDS[-4:]:
        res[f] &= (1 << 64) - 1
    return res
