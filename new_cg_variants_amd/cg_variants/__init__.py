"""Serial CG variants with the reference's call shape, computed on one MI355X.

    f(A, b, x0, max_iter, [preconditioner=...], callbacks=[], **kwargs) -> dict

mirrors numerical_experiments/cg_variants/__init__.py:64-74 (same names, argument
meaning and return value): ``A`` a SciPy CSR matrix, ``b``/``x0`` 1-D float64, the
result a dict with ``'name'``, ``'max_iter'`` and one length-``max_iter`` array per
recorder in ``callbacks`` (index 0 = initial state; ``max_iter - 1`` iterations run).
Inputs are not modified.  Breakdown (division by zero) yields inf/nan in the histories,
never an exception -- as in the reference.

Differences, all at the edges:
* the four standard recorders (see ``..callbacks``) are computed on the device; any
  other callable in ``callbacks`` is still honoured, called after every iteration with
  the reference's local names (``x_k``, ``r_k``, ``nu_k`` ...), at the price of a
  device->host copy of the state per iteration;
* ``preconditioner``: a callable that acts as a *diagonal* scaling (the reference's Jacobi
  lambda ``(1/A.diagonal())*x``, figure_gen.py:43, or the identity default) is probed once
  to recover the diagonal and then applied on the device; an object that carries ``bs`` and
  ``inv_blocks`` (``BlockJacobi(A, bs)``: the inverses of the bs x bs diagonal blocks, what
  PETSc calls pbjacobi) is applied on the device too, by a kernel of its own, and is never
  called (prcg.h: prcg_set_block_jacobi); ``DeviceBlockJacobi(A, bs)`` has the same blocks built on
  the device from the resident operator, without a host pass over the matrix (prcg.h:
  prcg_build_block_jacobi); ``VarBlockJacobi(A, block_ptr)`` and ``DeviceVarBlockJacobi(A, block_ptr)`` are the two
  for blocks of VARIABLE size that follow a partition (PETSc's vpbjacobi; prcg.h: prcg_set_block_jacobi_var,
  prcg_build_block_jacobi_var); any other callable is the caller's code, as it is
  in the reference, and is called on the host wherever the reference calls
  ``preconditioner(...)`` (prcg.h: prcg_set_preconditioner) while products, updates and
  inner products stay on the device;
* with an error recorder and no ``x_true`` the reference solves for it with a sparse direct
  solver on the fly (callbacks/error_A_norm.py:36-39); that is done here too up to n = 200,000
  -- beyond that it would never return, so the call asks for ``x_true`` instead.
"""
from collections import OrderedDict

import numpy as np

from .. import _lib as L
from ..callbacks import RECORDER_NAMES
from ..device import DeviceBatch, DeviceCSR, batch_matrices, batch_thresholds, batch_vectors, multi_rhs_shape_error

_OPERATORS = OrderedDict()   # small cache: figure_gen runs nine variants on one matrix
_PATTERNS = {}               # cache key -> fingerprint of indptr / indices alone (update_values finds an operator by its pattern)
_MAX_CACHED = 2
_MAX_DIRECT_SOLVE = 200_000   # largest system solved on the host for a missing x_true (the reference's on-the-fly spsolve)


def _fingerprint(A):
    """Content hash of the three CSR arrays, so that a matrix modified in place -- even by an edit
    that preserves sums -- is uploaded again instead of meeting a stale device operator."""
    try:
        import xxhash
        h = xxhash.xxh3_64()
        for a in (A.indptr, A.indices, A.data):
            h.update(np.ascontiguousarray(a).data)
        return h.intdigest()
    except ImportError:
        import zlib
        c = 0
        for a in (A.indptr, A.indices, A.data):
            c = zlib.crc32(np.ascontiguousarray(a).data, c)
        return c


def _pattern_fingerprint(A):
    """_fingerprint's hash over indptr and indices alone: what stays when only the values of a matrix change."""
    import zlib
    c = 0
    for a in (A.indptr, A.indices):
        c = zlib.crc32(np.ascontiguousarray(a).data, c)
    return c


def _operator(A, device):
    key = (id(A), A.shape, A.nnz, A.data.__array_interface__['data'][0], device, _fingerprint(A))
    op = _OPERATORS.get(key)
    if op is None:
        op = DeviceCSR(A, device=device)
        _OPERATORS[key] = op
        _PATTERNS[key] = _pattern_fingerprint(A)
        while len(_OPERATORS) > _MAX_CACHED:
            old_key, old = _OPERATORS.popitem(last=False)
            _PATTERNS.pop(old_key, None)
            old.close()
    else:
        _OPERATORS.move_to_end(key)
    return op


def clear_operator_cache():
    _PATTERNS.clear()
    while _OPERATORS:
        _, op = _OPERATORS.popitem()
        op.close()


def update_values(A, device=0):
    """After ``A.data`` has been modified IN PLACE (same indptr, indices: the same mesh with new coefficients), bring the
    cached device operator of ``A`` up to date instead of letting the next solve upload ``A`` as a second operator
    (DeviceCSR.update_values; prcg.h: prcg_update_values).  The operator is found by identity, shape, nnz and the
    fingerprint of indptr / indices kept beside the cache entry, and is re-keyed to the new content.  Returns the route
    taken, 'in_place' or 'replanned', or None if ``A`` has no cached operator on ``device`` -- the next solve then uploads
    it as it always has.  The reference has no counterpart: its functions read ``A`` anew at every call."""
    head = (id(A), A.shape, A.nnz, A.data.__array_interface__['data'][0], int(device))
    pattern = None
    for key in list(_OPERATORS):
        if key[:5] != head:
            continue
        if pattern is None:
            pattern = _pattern_fingerprint(A)
        if _PATTERNS.get(key) != pattern:
            continue
        op = _OPERATORS.pop(key)
        _PATTERNS.pop(key, None)
        try:
            route = op.update_values(np.ascontiguousarray(A.data, dtype=np.float64))
        except Exception:
            op.close()
            raise
        new_key = head + (_fingerprint(A),)
        stale = _OPERATORS.pop(new_key, None)
        if stale is not None:
            stale.close()
        _OPERATORS[new_key] = op
        _PATTERNS[new_key] = pattern
        return route
    return None


def _diagonal_of(preconditioner, n):
    """(d, None) with M^-1 v = d * v for a diagonal scaling (d None: the identity), or (None, preconditioner)
    for anything else.  The probe is exact for a diagonal scaling: M^-1 applied to ones IS d, bit for bit.
    A diagonal runs on the device; so does an object that carries `bs` and `inv_blocks` (BlockJacobi), which is
    handed on without a probe (_blocks_of; with bs == 1 it IS a diagonal); any other callable is called on the host
    wherever the reference calls `preconditioner(...)` -- it is the caller's code there too (prcg.h:
    prcg_set_preconditioner)."""
    if preconditioner is None:
        return None, None
    d = getattr(preconditioner, 'inv_diag', None)
    if d is not None:
        return L.f64(d), None
    blocks = _blocks_of(preconditioner)
    if blocks is not None:
        if blocks[0] == 1:
            return np.ascontiguousarray(blocks[1].reshape(-1)[:n]), None
        return None, preconditioner
    ones = np.ones(n)
    d = np.asarray(preconditioner(ones), dtype=np.float64)
    if d.shape != (n,):
        raise ValueError('preconditioner must map (n,) to (n,)')
    probe = np.random.default_rng(12345).standard_normal(n)
    if not np.array_equal(np.asarray(preconditioner(probe)), d * probe):
        return None, preconditioner
    if np.all(d == 1.0):
        return None, None
    return np.ascontiguousarray(d), None


def _blocks_of(preconditioner):
    """(bs, inv_blocks) of an object that carries them (device block Jacobi), else None."""
    bs, blocks = getattr(preconditioner, 'bs', None), getattr(preconditioner, 'inv_blocks', None)
    if bs is None or blocks is None:
        return None
    return int(bs), L.f64(blocks)


class Jacobi:
    """Jacobi preconditioner object: callable like the reference's lambda and carrying
    the reciprocal diagonal so no probing is needed."""

    def __init__(self, A):
        self.inv_diag = 1 / A.diagonal()          # figure_gen.py:43

    def __call__(self, v):
        return self.inv_diag * v


class BlockJacobi:
    """Point-block Jacobi preconditioner object (PETSc's pbjacobi; the reference has only the Jacobi lambda): the
    inverses of the bs x bs diagonal blocks of A, rows k*bs .. k*bs+bs-1 forming block k.  Passed as `preconditioner`
    to a *_pcg function it is applied on the device (prcg.h: prcg_set_block_jacobi) and never called; called, it
    evaluates the same arithmetic with NumPy multiplies and adds --

        acc = B[k][a][0] * v[k*bs];   acc = acc + B[k][a][j] * v[k*bs + j]   for j = 1, 2, ...

    -- so it serves any solver that takes a callable, with the same bits.  `inv_blocks`: (ceil(n/bs), bs, bs); a short
    last block (n not a multiple of bs) is inverted on its leading m x m part and padded with the identity."""

    _CHUNK = 1 << 22      # nonzeros gathered per step: bounds the temporaries on matrices with 10^8 nonzeros

    def __init__(self, A, bs):
        bs = int(bs)
        if not 1 <= bs <= 8:
            raise ValueError(f'BlockJacobi: block size {bs} outside 1..8')
        if A.format != 'csr':
            A = A.tocsr()
        n = A.shape[0]
        nb = -(-n // bs)
        self.bs, self.n = bs, n
        blocks = self._gather(A, n, nb, bs)
        m = n - bs * (nb - 1)                     # rows of the last block
        if m < bs and nb > 0:
            blocks[-1, np.arange(m, bs), np.arange(m, bs)] = 1.0
        bad = ~np.isfinite(blocks).all(axis=(1, 2))
        if bad.any():
            raise ValueError(f'BlockJacobi: diagonal block {int(np.argmax(bad))} (bs = {bs}) is not finite')
        try:
            inv = np.linalg.inv(blocks)
        except np.linalg.LinAlgError:
            raise ValueError(f'BlockJacobi: diagonal block {self._first_singular(blocks)} (bs = {bs}) is singular') from None
        bad = ~np.isfinite(inv).all(axis=(1, 2))
        if bad.any():
            raise ValueError(f'BlockJacobi: diagonal block {int(np.argmax(bad))} (bs = {bs}) is singular')
        if m < bs and nb > 0:                     # the short block: its own inverse, exact identity around it
            last = np.eye(bs)
            last[:m, :m] = np.linalg.inv(blocks[-1, :m, :m])
            inv[-1] = last
        self.inv_blocks = np.ascontiguousarray(inv)

    @classmethod
    def _gather(cls, A, n, nb, bs):
        """The diagonal blocks of CSR A as (nb, bs, bs), duplicates summed; chunks of rows, no loop over rows."""
        blocks = np.zeros((nb, bs, bs))
        indptr, indices, data = A.indptr, A.indices, A.data
        r0 = 0
        while r0 < n:
            r1 = int(np.searchsorted(indptr, indptr[r0] + cls._CHUNK, side='right')) - 1
            r1 = min(max(r1, r0 + 1), n)
            lo, hi = int(indptr[r0]), int(indptr[r1])
            rows = np.repeat(np.arange(r0, r1), np.diff(indptr[r0:r1 + 1]))
            cols = indices[lo:hi]
            keep = (cols // bs) == (rows // bs)
            rows, cols = rows[keep], cols[keep]
            np.add.at(blocks, (rows // bs, rows % bs, cols % bs), data[lo:hi][keep])
            r0 = r1
        return blocks

    @staticmethod
    def _first_singular(blocks):
        step = 4096
        for c0 in range(0, blocks.shape[0], step):
            try:
                np.linalg.inv(blocks[c0:c0 + step])
            except np.linalg.LinAlgError:
                for k in range(c0, min(c0 + step, blocks.shape[0])):
                    try:
                        np.linalg.inv(blocks[k])
                    except np.linalg.LinAlgError:
                        return k
        return -1

    def __call__(self, v):
        v = np.asarray(v, dtype=np.float64)
        bs, n = self.bs, self.n
        if v.shape != (n,):
            raise ValueError(f'BlockJacobi: expected a vector of {n} entries, got shape {v.shape}')
        nf = n // bs                               # full blocks
        out = np.empty(n)
        if nf:
            B, V = self.inv_blocks[:nf], v[:nf * bs].reshape(nf, bs)
            acc = B[:, :, 0] * V[:, 0:1]
            for j in range(1, bs):
                acc = acc + B[:, :, j] * V[:, j:j + 1]
            out[:nf * bs] = acc.reshape(-1)
        m = n - nf * bs
        if m:                                      # short last block: its m columns only
            B, V = self.inv_blocks[nf, :m, :m], v[nf * bs:]
            acc = B[:, 0] * V[0]
            for j in range(1, m):
                acc = acc + B[:, j] * V[j]
            out[nf * bs:] = acc
        return out


def invert_blocks(blocks):
    """The inversion loop of prcg_build_block_jacobi (prcg.h), restated with NumPy: Gauss-Jordan on [M | E], E = I, no pivoting,
    vectorised over the blocks, one ufunc per rounded operation -- for c = 0 .. bs-1: p = M[c][c]; row c of M and of E divided by
    p; every other row r: f = M[r][c], M[r] = M[r] - f * M[c], E[r] = E[r] - f * E[c].  ``blocks``: (nb, bs, bs), a short last
    block already inside its identity (what BlockJacobi._gather plus the padding gives).  Returns (inv, bad): E, which carries the
    bits of the device build for every block that is not bad, and the boolean mask of bad blocks -- a pivot zero or not finite at
    its step, or an entry of E not finite."""
    M = np.array(blocks, dtype=np.float64)
    if M.ndim != 3 or M.shape[1] != M.shape[2]:
        raise ValueError(f'invert_blocks: expected an array of shape (nb, bs, bs), got {M.shape}')
    nb, bs = M.shape[:2]
    E = np.broadcast_to(np.eye(bs), M.shape).copy()
    bad = np.zeros(nb, dtype=bool)
    with np.errstate(all='ignore'):
        for c in range(bs):
            p = M[:, c, c].copy()
            bad |= (p == 0.0) | ~np.isfinite(p)
            Mc, Ec = M[:, c, :] / p[:, None], E[:, c, :] / p[:, None]
            f = M[:, :, c].copy()
            M = M - f[:, :, None] * Mc[:, None, :]
            E = E - f[:, :, None] * Ec[:, None, :]
            M[:, c, :], E[:, c, :] = Mc, Ec             # the pivot row itself is scaled, not eliminated
        bad |= ~np.isfinite(E).all(axis=(1, 2))
    return E, bad


class DeviceBlockJacobi:
    """Point-block Jacobi whose inverses are BUILT ON THE DEVICE from the operator (prcg.h: prcg_build_block_jacobi): passed as
    `preconditioner` to a *_pcg function, the matrix is never touched on the host -- one kernel pass over the operator already
    resident gathers the bs x bs diagonal blocks, inverts them and leaves them where the apply kernel reads them; a later solve
    on the same operator reuses them, and a solve after update_values(A) builds them again.  The step after BlockJacobi for a
    Newton loop on an assembled matrix::

        A.data[:] = ...; update_values(A); pipe_pr_pcg(A, b, x0, max_iter, preconditioner=DeviceBlockJacobi(A, 3))

    The inversion is the fixed loop of prcg.h (Gauss-Jordan without pivoting: CG needs an SPD operator, whose diagonal blocks are
    SPD), not LAPACK's: the inverses differ from BlockJacobi's in the last bits, and a block such as [[0, 1], [1, 0]], which
    BlockJacobi inverts, is refused here (its first pivot is zero).  bs == 1 goes through the block kernel too.
    Called, the object builds `inv_blocks` on the host on first use -- BlockJacobi._gather plus invert_blocks, the restatement
    of the device loop, hence the bits the device uses -- from the values ``A`` holds at that moment, and applies them with
    BlockJacobi.__call__'s arithmetic: it serves the oracle and any solver that takes a callable.  A bad block raises
    ValueError('DeviceBlockJacobi: diagonal block K (bs = B) is singular or not finite') there as on the device path."""

    def __init__(self, A, bs):
        bs = int(bs)
        if not 1 <= bs <= 8:
            raise ValueError(f'DeviceBlockJacobi: block size {bs} outside 1..8')
        if A.format != 'csr':
            A = A.tocsr()
        self.A, self.bs, self.n = A, bs, A.shape[0]
        self._inv_blocks = None

    @property
    def inv_blocks(self):
        if self._inv_blocks is None:
            n, bs = self.n, self.bs
            nb = -(-n // bs)
            blocks = BlockJacobi._gather(self.A, n, nb, bs)
            m = n - bs * (nb - 1)
            if m < bs and nb > 0:
                blocks[-1, np.arange(m, bs), np.arange(m, bs)] = 1.0
            inv, bad = invert_blocks(blocks)
            if bad.any():
                raise ValueError(f'DeviceBlockJacobi: diagonal block {int(np.argmax(bad))} (bs = {bs}) is singular or not finite')
            self._inv_blocks = np.ascontiguousarray(inv)
        return self._inv_blocks

    def __call__(self, v):
        return BlockJacobi.__call__(self, v)


def _checked_partition(who, block_ptr, n):
    """block_ptr as int64, refused with the reasons of prcg_set_block_jacobi_var (prcg.h)"""
    ptr = np.ascontiguousarray(block_ptr, dtype=np.int64)
    if ptr.ndim != 1 or ptr.size < 1:
        raise ValueError(f'{who}: block_ptr must be a one-dimensional array of nb + 1 entries, got shape {ptr.shape}')
    if ptr[0] != 0:
        raise ValueError(f'{who}: block_ptr[0] is {int(ptr[0])}, not 0')
    if ptr[-1] != n:
        raise ValueError(f'{who}: block_ptr[nb] is {int(ptr[-1])}, not n_rows = {n}')
    sizes = np.diff(ptr)
    off = (sizes < 1) | (sizes > 8)
    if off.any():
        k = int(np.argmax(off))
        raise ValueError(f'{who}: block {k} has size {int(sizes[k])}, outside 1..8')
    return ptr


class VarBlockJacobi:
    """Point-block Jacobi with VARIABLE block sizes (PETSc's vpbjacobi): the inverses of the diagonal blocks of A that follow a
    partition -- block k owns rows and columns block_ptr[k] .. block_ptr[k+1]-1, every size in 1..8 -- for matrices whose nodes
    carry different numbers of unknowns (problems.fem_irregular_blocks gives the nodal partition of fem_irregular_3d).  As
    BlockJacobi: gathered on the host, inverted by LAPACK; passed as `preconditioner` to a *_pcg function it is applied on the
    device (prcg.h: prcg_set_block_jacobi_var) and never called; called, it evaluates the same arithmetic with NumPy --

        acc = B_k[a][0] * v[block_ptr[k]];   acc = acc + B_k[a][j] * v[block_ptr[k] + j]   for j = 1 .. m_k-1

    `inv_blocks`: PACKED, block k as m_k x m_k row-major at offset sum of m_q^2 over q < k; `block_ptr`; `n`."""

    _NAME = 'VarBlockJacobi'

    def __init__(self, A, block_ptr):
        if A.format != 'csr':
            A = A.tocsr()
        self.n = A.shape[0]
        self.block_ptr = _checked_partition(self._NAME, block_ptr, self.n)
        self._layout()
        packed = self._gather(A)
        inv = np.empty_like(packed)
        bad = np.zeros(self.block_ptr.size - 1, dtype=bool)
        with np.errstate(all='ignore'):
            for m, ks, at in self._groups:
                G = packed[at]
                fin = np.isfinite(G).all(axis=(1, 2))
                G = np.where(fin[:, None, None], G, np.eye(m))
                try:
                    E = np.linalg.inv(G)
                except np.linalg.LinAlgError:
                    E = np.full(G.shape, np.nan)
                    for q in range(G.shape[0]):
                        try:
                            E[q] = np.linalg.inv(G[q])
                        except np.linalg.LinAlgError:
                            pass
                bad[ks] = ~fin | ~np.isfinite(E).all(axis=(1, 2))
                inv[at] = E
        if bad.any():
            k = int(np.argmax(bad))
            raise ValueError(f'{self._NAME}: diagonal block {k} (size {int(self._sizes[k])}) is singular or not finite')
        self.inv_blocks = inv

    def _layout(self):
        """per block size m: the blocks of that size, and the index array (count, m, m) of their entries in the packed array"""
        ptr = self.block_ptr
        self._sizes = np.diff(ptr)
        self._offsets = np.concatenate([[0], np.cumsum(self._sizes ** 2)]).astype(np.int64)
        self._groups = []
        for m in range(1, 9):
            ks = np.flatnonzero(self._sizes == m)
            if ks.size:
                at = self._offsets[ks][:, None, None] + (np.arange(m)[:, None] * m + np.arange(m)[None, :])[None]
                self._groups.append((m, ks, at))

    def _gather(self, A):
        """The diagonal blocks of CSR A, packed: per row g = +0.0, then the row's entries whose column lies in the row's block
        added in CSR order (np.add.at adds one by one, in the order given) -- the gather of prcg_build_block_jacobi_var."""
        ptr, n = self.block_ptr, self.n
        packed = np.zeros(int(self._offsets[-1]))
        if n == 0:
            return packed
        block_of = np.repeat(np.arange(ptr.size - 1), self._sizes)
        indptr, indices, data = A.indptr, A.indices, A.data
        chunk, r0 = BlockJacobi._CHUNK, 0
        while r0 < n:
            r1 = int(np.searchsorted(indptr, indptr[r0] + chunk, side='right')) - 1
            r1 = min(max(r1, r0 + 1), n)
            lo, hi = int(indptr[r0]), int(indptr[r1])
            rows = np.repeat(np.arange(r0, r1), np.diff(indptr[r0:r1 + 1]))
            cols = indices[lo:hi].astype(np.int64)
            k = block_of[rows]
            keep = (cols >= ptr[k]) & (cols < ptr[k + 1])
            rows, cols, k = rows[keep], cols[keep], k[keep]
            np.add.at(packed, self._offsets[k] + (rows - ptr[k]) * self._sizes[k] + (cols - ptr[k]), data[lo:hi][keep])
            r0 = r1
        return packed

    def __call__(self, v):
        v = np.asarray(v, dtype=np.float64)
        if v.shape != (self.n,):
            raise ValueError(f'{self._NAME}: expected a vector of {self.n} entries, got shape {v.shape}')
        inv, out = self.inv_blocks, np.empty(self.n)
        for m, ks, at in self._groups:
            rows = self.block_ptr[ks][:, None] + np.arange(m)[None, :]
            B, V = inv[at], v[rows]
            acc = B[:, :, 0] * V[:, 0:1]
            for j in range(1, m):
                acc = acc + B[:, :, j] * V[:, j:j + 1]
            out[rows] = acc
        return out


class DeviceVarBlockJacobi(VarBlockJacobi):
    """VarBlockJacobi whose inverses are BUILT ON THE DEVICE from the operator (prcg.h: prcg_build_block_jacobi_var): passed as
    `preconditioner` to a *_pcg function, the matrix is never touched on the host; a later solve on the same operator with the
    same partition reuses the blocks, and a solve after update_values(A) builds them again -- DeviceBlockJacobi for a partition.
    The inversion is the fixed loop of prcg.h (Gauss-Jordan without pivoting, m_k steps on block k), not LAPACK's.
    Called, the object builds `inv_blocks` on the host on first use with the restatement of the device arithmetic -- the
    per-block gather in CSR order, then invert_blocks per group of equal size -- hence with the device's bits, from the values
    ``A`` holds at that moment.  A bad block raises ValueError('DeviceVarBlockJacobi: diagonal block K (size M) is singular or
    not finite') there as on the device path."""

    _NAME = 'DeviceVarBlockJacobi'

    def __init__(self, A, block_ptr):
        if A.format != 'csr':
            A = A.tocsr()
        self.A, self.n = A, A.shape[0]
        self.block_ptr = _checked_partition(self._NAME, block_ptr, self.n)
        self._inv_blocks = None

    @property
    def inv_blocks(self):
        if self._inv_blocks is None:
            self._layout()
            packed = self._gather(self.A)
            inv = np.empty_like(packed)
            bad = np.zeros(self.block_ptr.size - 1, dtype=bool)
            for m, ks, at in self._groups:
                inv[at], bad[ks] = invert_blocks(packed[at])
            if bad.any():
                k = int(np.argmax(bad))
                raise ValueError(f'{self._NAME}: diagonal block {k} (size {int(self._sizes[k])}) is singular or not finite')
            self._inv_blocks = inv
        return self._inv_blocks


_STATE_NAMES = {   # device vector -> the reference's local name
    'x': 'x_k', 'r': 'r_k', 'p': 'p_k', 's': 's_k', 'w': 'w_k', 'u': 'u_k',
    'rt': 'rt_k', 'st': 'st_k', 'wt': 'wt_k', 'ut': 'ut_k',
}


def _state_vectors(variant, prec):
    if variant == L.HS:
        return ['x', 'r', 'p', 's'] + (['rt'] if prec else [])
    if variant in (L.PR, L.M):
        return ['x', 'r', 'p', 's'] + (['rt', 'st'] if prec else [])
    if variant == L.CG_CG:
        return ['x', 'r', 'p', 's', 'w'] + (['rt'] if prec else [])
    if variant == L.GV:
        return ['x', 'r', 'p', 's', 'w', 'u'] + (['rt', 'wt', 'st'] if prec else [])
    return ['x', 'r', 'p', 's', 'w', 'u'] + (['rt', 'st', 'wt', 'ut'] if prec else [])


_PIPELINED = (L.PIPE_PR, L.PIPE_PR_M, L.PIPE_P, L.PIPE_P_M)


def _run(variant, name, A, b, x0, max_iter, preconditioner, callbacks, kwargs, w_replace=None, block_stop=False, hs_stop=False):
    """block_stop: the caller is a pipe_*_bpcg function, whose preconditioner is a block-Jacobi object: rtol= / atol= then reach the
    block session's own threshold (prcg.h: prcg_set_stop_block_jacobi) instead of being refused.
    hs_stop: the caller is hs_cg_stop / hs_pcg_stop: rtol= / atol= reach the Hestenes-Stiefel session's threshold (prcg.h:
    prcg_set_stop_hs), which serves no preconditioner but a diagonal scaling"""
    device = int(kwargs.get('device', 0))
    if A.format != 'csr':
        A = A.tocsr()
    n = A.shape[0]
    built = isinstance(preconditioner, DeviceBlockJacobi)      # blocks built on the device: the object is neither probed nor read
    var = isinstance(preconditioner, VarBlockJacobi)           # variable block sizes (either class): recognised before any probing
    if built or var:
        if preconditioner.n != n:
            raise ValueError(f'{type(preconditioner).__name__}: made for a matrix of {preconditioner.n} rows, the system has {n}')
        inv_diag, prec_fn = None, preconditioner
    else:
        inv_diag, prec_fn = _diagonal_of(preconditioner, n)
    if hs_stop and prec_fn is not None:
        raise ValueError(f'{name}: the function takes no preconditioner but a diagonal scaling (None, Jacobi(A), or a callable that is '
                         'one): a callable or block-Jacobi preconditioner runs the stored-tilde schedule with reduction launches, which '
                         'cannot stop on the device; use hs_pcg')
    # rtol= / atol=: the pipelined variants stop by themselves on the device (prcg.h: prcg_set_stop), and so do hs_cg_stop /
    # hs_pcg_stop (prcg_set_stop_hs); the other functions never took the keywords and keep passing them by, like any keyword they
    # do not know
    rr_stop = None
    if (variant in _PIPELINED or hs_stop) and (kwargs.get('rtol') is not None or kwargs.get('atol') is not None):
        bvec = np.asarray(b, dtype=np.float64)
        if bvec.shape != (n,):
            raise ValueError(f'{name}: b must have shape ({n},), got {tuple(bvec.shape)}')
        thr = _stop_thresholds(name, kwargs.pop('rtol', None), kwargs.pop('atol', None), [bvec])
        if thr is not None:
            if prec_fn is not None and not block_stop:
                raise ValueError(f'{name}: rtol= / atol= serve no preconditioner but a diagonal scaling: a callable or block-Jacobi '
                                 'preconditioner runs the stored-tilde schedule, which cannot stop on the device')
            rr_stop = float(thr[0])

    mask = 0
    foreign = []          # callables we must call ourselves, every iteration
    light = []            # host callbacks that need no vectors
    for cb in callbacks:
        cname = getattr(cb, 'prcg_recorder', None) or getattr(cb, '__name__', '')
        if cname in RECORDER_NAMES:
            mask |= L.HIST_BITS[cname]
        elif getattr(cb, 'prcg_host_light', False) or cname == 'pk':
            light.append(cb)
        else:
            foreign.append(cb)
    x_true = kwargs.get('x_true')
    if (mask & (L.HIST_ERROR_A_NORM | L.HIST_ERROR_2_NORM)) and x_true is None:
        # the reference solves for it on the fly (callbacks/error_A_norm.py:36-39)
        if n > _MAX_DIRECT_SOLVE:
            raise ValueError(f'error_A_norm / error_2_norm need x_true: solving the n = {n} system with a sparse direct solver on the '
                             f'host to obtain it (as the reference would) is not feasible beyond n = {_MAX_DIRECT_SOLVE}; pass x_true=')
        import scipy.sparse.linalg as spla
        x_true = spla.spsolve(A.tocsc().astype(np.double), np.asarray(b, dtype=np.double))
        kwargs['x_true'] = x_true

    op = _operator(A, device)
    output = {'name': name, 'max_iter': max_iter}
    if w_replace is not None:
        # gv_cg.py:9,69-71: the caller's predicate, with the reference's keywords; r_ is the residual of the previous iteration
        flags = {}
        prev = {'r': None}

        def hook(k):
            x, w, r = op.get_vector('x'), op.get_vector('w'), op.get_vector('r')
            if prev['r'] is None:
                prev['r'] = np.asarray(b, dtype=np.float64) - A @ np.asarray(x0, dtype=np.float64)
            fire = w_replace(k=k, A=A, b=b, x=x, w=w, r=r, r_=prev['r'], u=op.get_vector('u'), s=op.get_vector('s'),
                             p=op.get_vector('p'), wk_replace_flags=flags)
            prev['r'] = r
            return fire
        op.set_replace_hook(hook)
    else:
        op.set_replace_hook(None)
    blocks = _blocks_of(prec_fn) if prec_fn is not None and not built and not var else None
    if var:
        on_device = isinstance(preconditioner, DeviceVarBlockJacobi)       # built there: the object's blocks are never read
        try:
            op.begin(variant, b, x0, max_iter, x_true=x_true, hist_mask=mask, rr_stop=rr_stop,
                     block_jacobi_var=(preconditioner.block_ptr, None if on_device else preconditioner.inv_blocks))
        except ValueError as e:
            if 'diagonal block' not in str(e):
                raise
            raise ValueError('DeviceVarBlockJacobi: ' + str(e).split(': ', 1)[-1]) from None
    elif built:
        try:
            op.begin(variant, b, x0, max_iter, x_true=x_true, hist_mask=mask, block_jacobi=(preconditioner.bs, None), rr_stop=rr_stop)
        except ValueError as e:
            if 'diagonal block' not in str(e):
                raise
            raise ValueError('DeviceBlockJacobi: ' + str(e).split(': ', 1)[-1]) from None      # the library's text, this object's name
    elif blocks is not None:
        op.begin(variant, b, x0, max_iter, x_true=x_true, hist_mask=mask, block_jacobi=blocks, rr_stop=rr_stop)
    else:
        op.begin(variant, b, x0, max_iter, x_true=x_true, inv_diag=inv_diag, hist_mask=mask, preconditioner=prec_fn, rr_stop=rr_stop)

    def call_host(k):
        env = {'output': output, 'k': k, 'max_iter': max_iter, 'A': A, 'b': b, 'x0': x0, 'n': n,
               'kwargs': kwargs, 'callbacks': callbacks}
        for cb in light:
            cb(**env)
        if not foreign:
            return
        op.sync()
        for v in _state_vectors(variant, inv_diag is not None or prec_fn is not None):
            env[_STATE_NAMES[v]] = op.get_vector(v)
        sc = op.get_scalars(k)
        env.update(nu_k=sc[L.S_NU], mu_k=sc[L.S_MU], del_k=sc[L.S_DELTA], gam_k=sc[L.S_GAMMA])
        if variant in (L.CG_CG, L.GV):
            env['eta_k'] = sc[L.S_DELTA]          # slot 1 holds eta = w.r~ for these two
        with np.errstate(all='ignore'):
            env['a_k'] = sc[L.S_NU] / sc[L.S_MU]
        env['b_k'] = op.get_coefficients(k)[1] if k > 0 else 0
        for cb in foreign:
            cb(**env)

    def stopped():
        return rr_stop is not None and op.stop()[0] >= 0

    if foreign or light:
        call_host(0)
        for k in range(1, max_iter):
            if stopped():                  # the state of the stop iteration was the last one the callbacks saw
                break
            op.iterate(1)
            call_host(k)
    else:
        op.iterate(max_iter - 1)
    op.sync()
    output.update(op.history())
    if rr_stop is not None:
        k_stop, status = op.stop()
        output['iterations'] = k_stop if status else max_iter - 1
        output['status'] = ('max_iter', 'converged', 'breakdown')[status]
    return output


def _run_multi(variant, name, A, B, X0, max_iter, preconditioner, callbacks, kwargs):
    """Two or four right-hand sides of one matrix in ONE session of `variant` (L.HS, L.PR, L.M; prcg.h: prcg_solve_begin_multi; two
    of L.PIPE_PR, L.PIPE_PR_M: prcg_solve_begin_multi_pipe): what
    two (four) calls of hs_cg / hs_pcg (pr_cg / pr_pcg, m_cg / m_pcg) compute, with the operator streamed once per iteration for all of them.  Every argument is checked before
    the device is touched; what the session does not serve raises ValueError -- nothing falls back to two sessions."""
    if A.format != 'csr':
        A = A.tocsr()
    n = A.shape[0]
    B, X0 = np.asarray(B, dtype=np.float64), np.asarray(X0, dtype=np.float64)
    for nm, V, want in (('B', B, None), ('X0', X0, B.shape[0] if B.ndim == 2 else None)):
        err = multi_rhs_shape_error(nm, V.shape, n, want)
        if err:
            raise ValueError(f'{name}: {err}')
    nrhs = B.shape[0]
    pipelined = variant in (L.PIPE_PR, L.PIPE_PR_M)
    if pipelined and nrhs != 2:
        raise ValueError(f'{name}: B has shape {tuple(B.shape)}: the pipelined session serves exactly two right-hand sides, shape (2, {n}) '
                         '(its product is the four-vector one); solve four as two calls')
    for key in ('x_true', 'w_replace'):
        if kwargs.get(key) is not None:
            raise ValueError(f'{name}: {key} is not served by the two-RHS session')
    if isinstance(preconditioner, (DeviceBlockJacobi, VarBlockJacobi)):
        inv_diag, prec_fn = None, preconditioner
    else:
        inv_diag, prec_fn = _diagonal_of(preconditioner, n)
    if prec_fn is not None:
        kind = 'a block-Jacobi preconditioner' if isinstance(prec_fn, (DeviceBlockJacobi, VarBlockJacobi)) or _blocks_of(prec_fn) is not None else 'a preconditioner that is no diagonal scaling'
        hint = f"; blocks: {name.replace('_pcg_multi', '_bpcg_multi')}" if kind.startswith('a block') and name in ('hs_pcg_multi', 'pr_pcg_multi', 'm_pcg_multi') else ''
        raise ValueError(f'{name}: {kind} is not served by the two-RHS session (Jacobi(A), a callable that acts as a diagonal, or None{hint})')
    mask, light = _multi_callbacks(name, callbacks)
    # rtol= / atol=: the pipelined two-RHS session stops each column by itself on the device (prcg.h: prcg_set_stop_rhs); the other
    # multi-RHS functions never took the keywords and keep passing them by, like any keyword they do not know
    rr_stop = None
    if pipelined and (kwargs.get('rtol') is not None or kwargs.get('atol') is not None):
        rr_stop = _stop_thresholds(name, kwargs.pop('rtol', None), kwargs.pop('atol', None), [B[0], B[1]])
    op = _operator(A, int(kwargs.get('device', 0)))
    op.set_replace_hook(None)
    op.clear_preconditioners()            # (what an earlier solve left on the cached operator)
    if pipelined:
        op.begin_multi_pipe(variant, B, X0, max_iter, inv_diag=inv_diag, hist_mask=mask, rr_stop=rr_stop)
    else:
        op.begin_multi(variant, B, X0, max_iter, inv_diag=inv_diag, hist_mask=mask)
    return _multi_drive(op, name, A, B, X0, max_iter, light, callbacks, kwargs, stopping=rr_stop is not None)


def _multi_callbacks(name, callbacks):
    """(hist_mask, light host callbacks) of a multi-RHS session's callbacks; ValueError for what the session does not serve"""
    mask = 0
    light = []
    for cb in callbacks:
        cname = getattr(cb, 'prcg_recorder', None) or getattr(cb, '__name__', '')
        if cname == 'updated_residual_2_norm':
            mask |= L.HIST_BITS[cname]
        elif cname in RECORDER_NAMES:
            raise ValueError(f'{name}: recorder {cname} is not served by the two-RHS session (updated_residual_2_norm only)')
        elif getattr(cb, 'prcg_host_light', False) or cname == 'pk':
            light.append(cb)
        else:
            raise ValueError(f'{name}: callback {cname or cb!r} needs the state vectors every iteration: not served by the two-RHS '
                             'session (the updated_residual_2_norm recorder and light host callbacks are)')
    return mask, light


def _multi_drive(op, name, A, B, X0, max_iter, light, callbacks, kwargs, stopping=False):
    """run the multi-RHS session just begun on `op` to max_iter - 1 iterations; the list of per-column trial dicts.  stopping: the
    session was begun with per-column thresholds (begin_multi_pipe's rr_stop) -- a column's light host callbacks are called up to
    the iteration it stopped at and no further, the loop ends once every column has stopped, and each trial gains 'iterations'
    and 'status' (the words of the batch functions)."""
    n, nrhs = A.shape[0], B.shape[0]
    outputs = [{'name': name, 'max_iter': max_iter, 'rhs': j} for j in range(nrhs)]
    running = [True] * nrhs

    def call_host(k):
        for j in range(nrhs):
            if not running[j]:
                continue
            env = {'output': outputs[j], 'k': k, 'max_iter': max_iter, 'A': A, 'b': B[j], 'x0': X0[j], 'n': n,
                   'kwargs': kwargs, 'callbacks': callbacks}
            for cb in light:
                cb(**env)

    def update_running():                  # the state of its stop iteration was the last one a column's callbacks saw
        if stopping:
            for j, (k_stop, _) in enumerate(op.stops_rhs()):
                running[j] = k_stop < 0

    if light:
        call_host(0)
        for k in range(1, max_iter):
            update_running()
            if not any(running):
                break
            op.iterate(1)
            call_host(k)
    else:
        op.iterate(max_iter - 1)
    op.sync()
    for j in range(nrhs):
        outputs[j].update(op.history(rhs=j))
    if stopping:
        for j, (k_stop, status) in enumerate(op.stops_rhs()):
            outputs[j]['iterations'] = k_stop if status else max_iter - 1
            outputs[j]['status'] = ('max_iter', 'converged', 'breakdown')[status]
    return outputs


def _run_multi_blocks(variant, name, A, B, X0, max_iter, preconditioner, callbacks, kwargs):
    """Two or four right-hand sides of one matrix in ONE session of `variant` (L.HS, L.PR, L.M) preconditioned by point-block Jacobi on
    the device (prcg.h: prcg_solve_begin_multi_block_jacobi).  Shapes, callbacks, x_true and w_replace are checked as _run_multi checks
    them, before the device is touched; a preconditioner that carries no blocks raises ValueError naming the function to use."""
    if A.format != 'csr':
        A = A.tocsr()
    n = A.shape[0]
    B, X0 = np.asarray(B, dtype=np.float64), np.asarray(X0, dtype=np.float64)
    for nm, V, want in (('B', B, None), ('X0', X0, B.shape[0] if B.ndim == 2 else None)):
        err = multi_rhs_shape_error(nm, V.shape, n, want)
        if err:
            raise ValueError(f'{name}: {err}')
    for key in ('x_true', 'w_replace'):
        if kwargs.get(key) is not None:
            raise ValueError(f'{name}: {key} is not served by the two-RHS session')
    other = name.replace('_bpcg_multi', '_pcg_multi')
    built = isinstance(preconditioner, DeviceBlockJacobi)
    var = isinstance(preconditioner, VarBlockJacobi)
    blocks = None if built or var or preconditioner is None else _blocks_of(preconditioner)
    if not (built or var) and (blocks is None or getattr(preconditioner, 'inv_diag', None) is not None):
        what = ('no preconditioner' if preconditioner is None else
                'a diagonal scaling' if getattr(preconditioner, 'inv_diag', None) is not None else 'a preconditioner that carries no blocks')
        raise ValueError(f'{name}: {what}: the block session takes BlockJacobi, DeviceBlockJacobi, VarBlockJacobi, DeviceVarBlockJacobi or an '
                         f'object carrying bs / inv_blocks; use {other} (Jacobi(A), a callable that acts as a diagonal, or None)')
    if (built or var) and preconditioner.n != n:
        raise ValueError(f'{type(preconditioner).__name__}: made for a matrix of {preconditioner.n} rows, the system has {n}')
    if blocks is not None and (not 1 <= blocks[0] <= 8 or blocks[1].shape != (-(-n // blocks[0]), blocks[0], blocks[0])):
        raise ValueError(f'{name}: need 1 <= bs <= 8 and inv_blocks of shape (ceil(n/bs), bs, bs); got bs={blocks[0]}, {blocks[1].shape}')
    mask, light = _multi_callbacks(name, callbacks)
    op = _operator(A, int(kwargs.get('device', 0)))
    op.set_replace_hook(None)
    try:
        if var:
            on_device = isinstance(preconditioner, DeviceVarBlockJacobi)       # built there: the object's blocks are never read
            op.begin_multi_block_jacobi(variant, B, X0, max_iter, hist_mask=mask,
                                        block_jacobi_var=(preconditioner.block_ptr, None if on_device else preconditioner.inv_blocks))
        elif built:
            op.begin_multi_block_jacobi(variant, B, X0, max_iter, hist_mask=mask, block_jacobi=(preconditioner.bs, None))
        else:
            op.begin_multi_block_jacobi(variant, B, X0, max_iter, hist_mask=mask, block_jacobi=blocks)
    except ValueError as e:
        if 'diagonal block' not in str(e) or not (built or var):
            raise
        raise ValueError(f'{type(preconditioner).__name__}: ' + str(e).split(': ', 1)[-1]) from None      # the library's text, this object's name
    return _multi_drive(op, name, A, B, X0, max_iter, light, callbacks, kwargs)


def _make_bpcg_multi(variant, name, where):
    single = name[:-len('_bpcg_multi')]

    def f(A, B, X0, max_iter, preconditioner, callbacks=[], **kwargs):
        return _run_multi_blocks(variant, name, A, B, X0, max_iter, preconditioner, callbacks, kwargs)
    f.__doc__ = (f'{single}_pcg ({where}) for TWO or FOUR right-hand sides of one matrix, preconditioned by POINT-BLOCK JACOBI applied on the '
                 'device: B, X0 of shape (2, n) or (4, n); returns a list of two or four trial dicts.  preconditioner: BlockJacobi, '
                 'DeviceBlockJacobi, VarBlockJacobi, DeviceVarBlockJacobi or an object carrying bs / inv_blocks; None, a diagonal or any '
                 f'other callable is a ValueError naming {single}_pcg_multi.  One session (prcg.h: prcg_solve_begin_multi_block_jacobi): per '
                 'iteration one pass over the operator for all systems and one pass over the blocks per pair of systems, with the inner '
                 'products that need M^-1 formed in the launch that applies it.')
    f.__name__ = f.__qualname__ = name
    return f


hs_bpcg_multi = _make_bpcg_multi(L.HS, 'hs_bpcg_multi', 'hs_cg.py:70')
pr_bpcg_multi = _make_bpcg_multi(L.PR, 'pr_bpcg_multi', 'pr_cg.py:166')
m_bpcg_multi = _make_bpcg_multi(L.M, 'm_bpcg_multi', 'pr_cg.py:172')


def hs_cg_multi(A, B, X0, max_iter, callbacks=[], **kwargs):
    """hs_cg (hs_cg.py:9) for TWO or FOUR right-hand sides of one matrix: B, X0 of shape (2, n) or (4, n); returns a list of
    two or four trial dicts shaped like hs_cg's.  One session, one pass over the operator per iteration."""
    if kwargs.pop('preconditioner', None) is not None:
        raise ValueError('hs_cg_multi takes no preconditioner: use hs_pcg_multi')
    return _run_multi(L.HS, 'hs_cg_multi', A, B, X0, max_iter, None, callbacks, kwargs)


def hs_pcg_multi(A, B, X0, max_iter, preconditioner=None, callbacks=[], **kwargs):
    """hs_pcg (hs_cg.py:70) for TWO or FOUR right-hand sides of one matrix, with Jacobi(A) or a callable that probes as a diagonal."""
    return _run_multi(L.HS, 'hs_pcg_multi', A, B, X0, max_iter, preconditioner, callbacks, kwargs)


def _make_multi(variant, name, preconditioned):
    single = name[:-len('_multi')]
    if preconditioned:
        def f(A, B, X0, max_iter, preconditioner=None, callbacks=[], **kwargs):
            return _run_multi(variant, name, A, B, X0, max_iter, preconditioner, callbacks, kwargs)
        f.__doc__ = (f'{single} (pr_cg.py:{166 if variant == L.PR else 172}) for TWO or FOUR right-hand sides of one matrix, with Jacobi(A) or a '
                     'callable that probes as a diagonal: B, X0 of shape (2, n) or (4, n); returns a list of two or four trial dicts.  One session, one '
                     'pass over the operator and one reduction point per iteration.')
    else:
        def f(A, B, X0, max_iter, callbacks=[], **kwargs):
            if kwargs.pop('preconditioner', None) is not None:
                raise ValueError(f'{name} takes no preconditioner: use {single[:-2]}pcg_multi')
            return _run_multi(variant, name, A, B, X0, max_iter, None, callbacks, kwargs)
        f.__doc__ = (f'{single} (the identity-preconditioned recurrence of {single[:-2]}pcg) for TWO or FOUR right-hand sides of one matrix: B, X0 '
                     'of shape (2, n) or (4, n); returns a list of two or four trial dicts.  One session, one pass over the operator per iteration.')
    f.__name__ = f.__qualname__ = name
    return f


pr_cg_multi = _make_multi(L.PR, 'pr_cg_multi', False)
pr_pcg_multi = _make_multi(L.PR, 'pr_pcg_multi', True)       # pr_cg.py:166
m_cg_multi = _make_multi(L.M, 'm_cg_multi', False)
m_pcg_multi = _make_multi(L.M, 'm_pcg_multi', True)          # pr_cg.py:172


def _make_multi_pipe(variant, name, preconditioned, line):
    single = name[:-len('_multi')]
    doc = (f'{single} (pipe_pr_cg.py:{line}) for TWO right-hand sides of one matrix: B, X0 of shape (2, n); returns a list of two trial dicts '
           f'shaped like {single}\'s.  One pipelined session (prcg.h: prcg_solve_begin_multi_pipe): per iteration one update launch for both '
           'systems and ONE product of four vectors, so the operator is streamed once for both.  Prefer it where the operator dominates an '
           'iteration\'s traffic (assembled FEM matrices); on band and stencil operators two calls of the single function, one launch per '
           'iteration each, may be faster (profiles/multi_rhs_pipe.md).  (4, n) is refused: nothing falls back to two sessions.  '
           'rtol= / atol= (one value, or one per system): each system stops by itself on the device at r.r <= max(rtol ||b||, atol)^2 or '
           'on breakdown (prcg.h: prcg_set_stop_rhs) while the other runs on; each trial then carries \'iterations\' and \'status\' '
           '(\'converged\' / \'breakdown\' / \'max_iter\') and its history is zero beyond its stop.')
    if preconditioned:
        def f(A, B, X0, max_iter, preconditioner=None, callbacks=[], **kwargs):
            return _run_multi(variant, name, A, B, X0, max_iter, preconditioner, callbacks, kwargs)
        f.__doc__ = doc + '  preconditioner: Jacobi(A), a callable that probes as a diagonal, or None.'
    else:
        def f(A, B, X0, max_iter, callbacks=[], **kwargs):
            if kwargs.pop('preconditioner', None) is not None:
                raise ValueError(f'{name} takes no preconditioner: use {single[:-2]}pcg_multi')
            return _run_multi(variant, name, A, B, X0, max_iter, None, callbacks, kwargs)
        f.__doc__ = doc
    f.__name__ = f.__qualname__ = name
    return f


pipe_pr_cg_multi = _make_multi_pipe(L.PIPE_PR, 'pipe_pr_cg_multi', False, 89)
pipe_pr_pcg_multi = _make_multi_pipe(L.PIPE_PR, 'pipe_pr_pcg_multi', True, 201)
pipe_pr_m_cg_multi = _make_multi_pipe(L.PIPE_PR_M, 'pipe_pr_m_cg_multi', False, 101)
pipe_pr_m_pcg_multi = _make_multi_pipe(L.PIPE_PR_M, 'pipe_pr_m_pcg_multi', True, 213)


def _batch_diagonals(name, preconditioner, sizes):
    """The systems' reciprocal diagonals, one vector per system, from the `preconditioner` of a *_pcg_batch function: one
    object (every system uses it: the sizes must agree) or a sequence with one per system, each resolved with the rule of
    _diagonal_of; None -- the whole argument or an entry -- is the identity (ones), as the reference's *_pcg without a
    preconditioner.  Host work only; ValueError for anything that is not a diagonal scaling."""
    n_sys = len(sizes)

    def resolve(prec, n, where):
        if prec is None:
            return np.ones(n)
        if not callable(prec) and getattr(prec, 'inv_diag', None) is None and _blocks_of(prec) is None:
            raise ValueError(f'{name}: {where} is neither callable nor carries inv_diag: a batch applies diagonal preconditioners only')
        d, fn = _diagonal_of(prec, n)
        if fn is not None:
            raise ValueError(f'{name}: {where} is not a diagonal scaling: a batch applies diagonal preconditioners only '
                             '(Jacobi, a callable v -> d * v, or block Jacobi with bs == 1)')
        if d is None:
            return np.ones(n)
        d = np.asarray(d, dtype=np.float64)
        if d.shape != (n,):
            raise ValueError(f'{name}: {where} carries a diagonal of shape {tuple(d.shape)}, the system has size {n}')
        return d
    if isinstance(preconditioner, (list, tuple)):
        if len(preconditioner) != n_sys:
            raise ValueError(f'{name}: preconditioner must be one object or a sequence of {n_sys}, one per system -- got {len(preconditioner)}')
        return [resolve(prec, n, f'preconditioner[{s}]') for s, (prec, n) in enumerate(zip(preconditioner, sizes))]
    if preconditioner is not None and len(set(sizes)) != 1:
        raise ValueError(f'{name}: one preconditioner object for {n_sys} systems of different sizes {sorted(set(sizes))}: pass a sequence '
                         'with one per system')
    d = resolve(preconditioner, sizes[0], 'preconditioner') if preconditioner is not None else None
    return [np.ones(n) if d is None else d for n in sizes]


def _batch_blocks(name, preconditioner, sizes):
    """The systems' partitions and packed inverses, one pair (block_ptr, inv_blocks) per system (DeviceBatch.begin's
    block_jacobi), from the `preconditioner` of a *_bpcg_batch function: one object (every system uses it: the sizes must agree)
    or a sequence with one per system.  An object carrying block_ptr / inv_blocks (VarBlockJacobi) is taken as it is; one
    carrying bs / inv_blocks (BlockJacobi: (ceil(n/bs), bs, bs), the short last block inside an identity) becomes the partition
    0, bs, 2 bs, ..., n with the last block cut to its m x m part; an object carrying inv_diag (Jacobi) or a callable that the
    exact probe of _diagonal_of shows to be v -> d * v is a partition of ones; None is the identity.  Host work only; ValueError
    for anything else, for a partition prcg_batch_begin_block_jacobi would refuse and for blocks that do not match the system."""
    n_sys = len(sizes)

    def resolve(prec, n, where):
        if prec is None:
            return np.arange(n + 1, dtype=np.int64), np.ones(n)
        inv = getattr(prec, 'inv_blocks', None)
        if inv is not None and getattr(prec, 'block_ptr', None) is not None:
            ptr = np.ascontiguousarray(prec.block_ptr, dtype=np.int64)
            if ptr.ndim == 1 and ptr.size and ptr[-1] != n:
                raise ValueError(f'{name}: {where} carries a partition of {int(ptr[-1])} rows, the system has size {n}')
            ptr = _checked_partition(f'{name}: {where}', ptr, n)
            inv = L.f64(inv).reshape(-1)
            if inv.size != int(np.sum(np.diff(ptr) ** 2)):
                raise ValueError(f'{name}: {where} carries {inv.size} entries of inv_blocks, its partition needs '
                                 f'{int(np.sum(np.diff(ptr) ** 2))} (packed: block k is m_k x m_k)')
            return ptr, inv
        if inv is not None and getattr(prec, 'bs', None) is not None:
            bs, inv = int(prec.bs), L.f64(inv)
            if not 1 <= bs <= 8:
                raise ValueError(f'{name}: {where} has block size {bs}, outside 1..8')
            nb = -(-n // bs)
            if inv.shape != (nb, bs, bs):
                raise ValueError(f'{name}: {where} carries inv_blocks of shape {tuple(inv.shape)}, a system of size {n} with bs = {bs} '
                                 f'has ({nb}, {bs}, {bs})')
            ptr = np.minimum(np.arange(nb + 1, dtype=np.int64) * bs, n)
            m = n - bs * (nb - 1)
            return ptr, np.concatenate([inv[:nb - 1].reshape(-1), inv[nb - 1, :m, :m].reshape(-1)])
        if not callable(prec) and getattr(prec, 'inv_diag', None) is None:
            raise ValueError(f'{name}: {where} is neither a block-Jacobi object (bs / inv_blocks or block_ptr / inv_blocks), nor carries '
                             'inv_diag, nor is callable')
        d, fn = _diagonal_of(prec, n)
        if fn is not None:
            raise ValueError(f'{name}: {where} is a callable that is not a diagonal scaling: a batch applies block Jacobi (BlockJacobi, '
                             'VarBlockJacobi), Jacobi or a callable v -> d * v')
        d = np.ones(n) if d is None else np.asarray(d, dtype=np.float64)
        if d.shape != (n,):
            raise ValueError(f'{name}: {where} carries a diagonal of shape {tuple(d.shape)}, the system has size {n}')
        return np.arange(n + 1, dtype=np.int64), d
    if isinstance(preconditioner, (list, tuple)):
        if len(preconditioner) != n_sys:
            raise ValueError(f'{name}: preconditioner must be one object or a sequence of {n_sys}, one per system -- got {len(preconditioner)}')
        return [resolve(prec, n, f'preconditioner[{s}]') for s, (prec, n) in enumerate(zip(preconditioner, sizes))]
    if preconditioner is not None and len(set(sizes)) != 1:
        raise ValueError(f'{name}: one preconditioner object for {n_sys} systems of different sizes {sorted(set(sizes))}: pass a sequence '
                         'with one per system')
    if preconditioner is None:
        return [resolve(None, n, 'preconditioner') for n in sizes]
    return [resolve(preconditioner, sizes[0], 'preconditioner')] * n_sys


def _stop_thresholds(name, rtol, atol, rhs):
    """rtol / atol (each None, one value, or one value per system) -> the thresholds on r.r the device stops at, one per
    right-hand side in ``rhs``: thr_s = max(rtol_s ||b_s||_2, atol_s)^2; None when neither is given.  Shared by the batches and
    the pipelined single functions (one system).  Pure host work; ValueError names the function, the keyword and the system."""
    if rtol is None and atol is None:
        return None
    n_sys = len(rhs)
    try:
        rt = batch_thresholds('rtol', 0.0 if rtol is None else rtol, n_sys)
        ab = batch_thresholds('atol', 0.0 if atol is None else atol, n_sys)
    except ValueError as e:
        raise ValueError(f'{name}: {e}') from None
    norms = np.array([np.linalg.norm(b) for b in rhs])
    rr_stop = np.maximum(rt * norms, ab) ** 2
    try:
        return batch_thresholds('max(rtol * ||b||, atol) ** 2', rr_stop, n_sys)
    except ValueError as e:
        raise ValueError(f'{name}: {e}') from None


def _run_batch(variant, name, As, bs, x0s, max_iter, callbacks, kwargs, jacobi=False, blocks=False):
    """A batch of small independent systems in ONE launch, one workgroup per system (prcg.h: prcg_batch_create): what a loop
    of `name`'s single function over the systems computes.  Every argument is checked before the device is touched; what the
    batch does not serve raises ValueError -- nothing falls back to a loop of sessions.  jacobi: a *_pcg_batch function,
    kwargs['preconditioner'] resolved to one reciprocal diagonal per system (prcg.h: prcg_batch_begin_jacobi); blocks: a
    *_bpcg_batch function, resolved to one partition with its inverses per system (prcg.h: prcg_batch_begin_block_jacobi)."""
    preconditioner = kwargs.pop('preconditioner', None)
    rtol, atol = kwargs.pop('rtol', None), kwargs.pop('atol', None)
    if not jacobi and not blocks and preconditioner is not None:
        raise ValueError(f'{name} takes no preconditioner: a batch runs the unpreconditioned one-workgroup solver')
    for key in ('x_true', 'w_replace'):
        if kwargs.get(key) is not None:
            raise ValueError(f'{name}: {key} is not served by a batch')
    n_sys = bs.shape[0] if isinstance(bs, np.ndarray) and bs.ndim == 2 else len(bs)
    try:
        matrices, mat_of = batch_matrices(As, n_sys)
    except ValueError as e:
        raise ValueError(f'{name}: {e}') from None
    matrices = [A if A.format == 'csr' else A.tocsr() for A in matrices]
    sizes = [matrices[m].shape[0] for m in mat_of]
    try:
        B, X0 = batch_vectors('bs', bs, sizes), batch_vectors('x0s', x0s, sizes)
    except ValueError as e:
        raise ValueError(f'{name}: {e}') from None
    mask = 0
    for cb in callbacks:
        cname = getattr(cb, 'prcg_recorder', None) or getattr(cb, '__name__', '')
        if cname == 'updated_residual_2_norm':
            mask |= L.HIST_BITS[cname]
        else:
            raise ValueError(f'{name}: callback {cname or repr(cb)} is not served by a batch (the updated_residual_2_norm recorder or none)')
    inv_diag = _batch_diagonals(name, preconditioner, sizes) if jacobi else None
    block_jacobi = _batch_blocks(name, preconditioner, sizes) if blocks else None
    at = np.concatenate([[0], np.cumsum(sizes)])
    rr_stop = _stop_thresholds(name, rtol, atol, [B[at[s]:at[s + 1]] for s in range(n_sys)])
    batch = DeviceBatch(matrices, mat_of, device=int(kwargs.get('device', 0)))
    try:
        batch.begin(variant, [B[at[s]:at[s + 1]] for s in range(n_sys)], [X0[at[s]:at[s + 1]] for s in range(n_sys)], max_iter, hist_mask=mask,
                    inv_diag=inv_diag, rr_stop=rr_stop, block_jacobi=block_jacobi)
        batch.iterate(max_iter - 1)
        batch.sync()
        outputs = [{'name': name, 'max_iter': max_iter, 'system': s} for s in range(n_sys)]
        for s in range(n_sys):
            outputs[s].update(batch.history(s))
        if rr_stop is not None:
            k_stop, status = batch.stops()
            for s in range(n_sys):
                outputs[s]['iterations'] = int(k_stop[s]) if status[s] else max_iter - 1
                outputs[s]['status'] = ('max_iter', 'converged', 'breakdown')[int(status[s])]
    finally:
        batch.close()
    return outputs


def _make_batch(variant, name, where):
    single = name[:-len('_batch')]

    def f(As, bs, x0s, max_iter, callbacks=[], **kwargs):
        return _run_batch(variant, name, As, bs, x0s, max_iter, callbacks, kwargs)
    f.__doc__ = (f'{single} ({where}) for a BATCH of small independent systems, all solved in one launch, one workgroup per system: As is one '
                 'matrix (every system uses it) or a sequence as long as bs (entries that are the same object share one upload); bs, x0s are '
                 f'lists of vectors or, when all sizes agree, 2-D arrays.  Returns a list of trial dicts, one per system, shaped like {single}\'s.  '
                 'callbacks: updated_residual_2_norm or none.  Every system must fit the one-workgroup solver (n <= 4096, matrix in registers '
                 'or LDS): anything else is refused.  rtol= and/or atol= (a scalar, or one value per system): every system stops by itself '
                 'once its updated residual satisfies r.r <= max(rtol ||b||_2, atol)^2, or at a breakdown (prcg.h: prcg_batch_set_stop); each '
                 'trial dict then carries \'iterations\' (the stop iteration, max_iter - 1 for a system that ran out) and \'status\' '
                 '(\'converged\', \'breakdown\', \'max_iter\'), and the history is zero beyond the stop.')
    f.__name__ = f.__qualname__ = name
    return f


pipe_pr_cg_batch = _make_batch(L.PIPE_PR, 'pipe_pr_cg_batch', 'pipe_pr_cg.py:89')
pipe_pr_m_cg_batch = _make_batch(L.PIPE_PR_M, 'pipe_pr_m_cg_batch', 'pipe_pr_cg.py:101')
hs_cg_batch = _make_batch(L.HS, 'hs_cg_batch', 'hs_cg.py:9')


def _make_pcg_batch(variant, name, where):
    single = name[:-len('_batch')]

    def f(As, bs, x0s, max_iter, preconditioner=None, callbacks=[], **kwargs):
        kwargs['preconditioner'] = preconditioner
        return _run_batch(variant, name, As, bs, x0s, max_iter, callbacks, kwargs, jacobi=True)
    f.__doc__ = (f'{single} ({where}) for a BATCH of small independent systems, all solved in one launch, one workgroup per system, the '
                 f'preconditioner applied inside it.  As, bs, x0s, callbacks and the result as {single[:-3]}cg_batch.  preconditioner: one object '
                 '(every system uses it: the sizes must agree) or a sequence with one per system; each must be a DIAGONAL scaling -- an object '
                 'carrying inv_diag (Jacobi), block Jacobi with bs == 1, or a callable that the exact probe shows to be v -> d * v --, anything '
                 'else is a ValueError; None is the identity, as the reference\'s function without a preconditioner.  rtol= / atol= as '
                 f'{single[:-3]}cg_batch.')
    f.__name__ = f.__qualname__ = name
    return f


pipe_pr_pcg_batch = _make_pcg_batch(L.PIPE_PR, 'pipe_pr_pcg_batch', 'pipe_pr_cg.py:201')
pipe_pr_m_pcg_batch = _make_pcg_batch(L.PIPE_PR_M, 'pipe_pr_m_pcg_batch', 'pipe_pr_cg.py:213')
hs_pcg_batch = _make_pcg_batch(L.HS, 'hs_pcg_batch', 'hs_cg.py:70')


def _make_bpcg_batch(variant, name, where):
    single = name[:-len('_bpcg_batch')]

    def f(As, bs, x0s, max_iter, preconditioner=None, callbacks=[], **kwargs):
        kwargs['preconditioner'] = preconditioner
        return _run_batch(variant, name, As, bs, x0s, max_iter, callbacks, kwargs, blocks=True)
    f.__doc__ = (f'{single}_pcg ({where}) for a BATCH of small independent systems, all solved in one launch, one workgroup per system, '
                 f'preconditioned by POINT-BLOCK JACOBI applied inside it.  As, bs, x0s, callbacks, rtol= / atol= and the result as '
                 f'{single}_pcg_batch.  preconditioner: one object (every system uses it: the sizes must agree) or a sequence with one per '
                 'system -- BlockJacobi, VarBlockJacobi (or any object carrying bs / inv_blocks or block_ptr / inv_blocks; every block size in '
                 '1..8); Jacobi or a callable v -> d * v is a partition of ones; None is the identity; anything else is a ValueError.  A '
                 'system that fits the one-workgroup solver with a diagonal scaling fits it with blocks (prcg.h: '
                 'prcg_batch_begin_block_jacobi).')
    f.__name__ = f.__qualname__ = name
    return f


pipe_pr_bpcg_batch = _make_bpcg_batch(L.PIPE_PR, 'pipe_pr_bpcg_batch', 'pipe_pr_cg.py:201')
pipe_pr_m_bpcg_batch = _make_bpcg_batch(L.PIPE_PR_M, 'pipe_pr_m_bpcg_batch', 'pipe_pr_cg.py:213')
hs_bpcg_batch = _make_bpcg_batch(L.HS, 'hs_bpcg_batch', 'hs_cg.py:70')


def _make(variant, name, preconditioned):
    def take_w_replace(kwargs):
        # gv_cg.py:9 / :93 take a residual-replacement predicate (default: never); the other variants swallow the keyword
        fn = kwargs.pop('w_replace', None)
        return fn if variant == L.GV else None
    if preconditioned:
        def f(A, b, x0, max_iter, preconditioner=None, callbacks=[], **kwargs):
            w_replace = take_w_replace(kwargs)
            return _run(variant, name, A, b, x0, max_iter, preconditioner, callbacks, kwargs, w_replace)
    else:
        def f(A, b, x0, max_iter, callbacks=[], **kwargs):
            w_replace = take_w_replace(kwargs)
            kwargs.pop('preconditioner', None)   # figure_gen.py:59 always passes one
            return _run(variant, name, A, b, x0, max_iter, None, callbacks, kwargs, w_replace)
    f.__name__ = f.__qualname__ = name
    return f


def _make_bpcg(variant, name, where):
    single = name[:-len('_bpcg')]

    def f(A, b, x0, max_iter, preconditioner, callbacks=[], rtol=None, atol=None, **kwargs):
        if not isinstance(preconditioner, (BlockJacobi, DeviceBlockJacobi, VarBlockJacobi)):
            what = ('no preconditioner' if preconditioner is None else
                    'a diagonal scaling' if getattr(preconditioner, 'inv_diag', None) is not None else f'a {type(preconditioner).__name__}')
            raise ValueError(f'{name}: {what}: the function takes BlockJacobi, DeviceBlockJacobi, VarBlockJacobi or DeviceVarBlockJacobi; use '
                             f'{single}_pcg (Jacobi(A), any callable, or None)')
        kwargs.pop('w_replace', None)
        if rtol is not None or atol is not None:
            kwargs.update(rtol=rtol, atol=atol)
        return _run(variant, name, A, b, x0, max_iter, preconditioner, callbacks, kwargs, block_stop=True)
    f.__doc__ = (f'{single}_pcg ({where}) preconditioned by POINT-BLOCK JACOBI applied on the device, in a session that can STOP by itself.  '
                 'preconditioner: BlockJacobi, DeviceBlockJacobi, VarBlockJacobi or DeviceVarBlockJacobi; anything else is a ValueError before '
                 f'the device is reached.  Without rtol= / atol= the result is {single}_pcg\'s with the same object, bit for bit.  rtol= and/or '
                 'atol=: the session stops on the device once its updated residual satisfies r.r <= max(rtol ||b||_2, atol)^2, or at a '
                 'breakdown (prcg.h: prcg_set_stop_block_jacobi); the trial dict then carries \'iterations\' and \'status\' (\'converged\' / '
                 '\'breakdown\' / \'max_iter\'), histories are zero beyond the stop and callbacks are called up to the stop iteration and no '
                 f'further.  ({single}_pcg keeps refusing rtol= / atol= with such an object.)')
    f.__name__ = f.__qualname__ = name
    return f


hs_cg = _make(L.HS, 'hs_cg', False)                       # hs_cg.py:9
hs_pcg = _make(L.HS, 'hs_pcg', True)                      # hs_cg.py:70
hs_cg.__doc__ = ('hs_cg (hs_cg.py:9): max_iter - 1 iterations.  rtol= / atol= are passed by like any keyword the reference does not know; '
                 'hs_cg_stop takes them and stops on the device.')
hs_pcg.__doc__ = ('hs_pcg (hs_cg.py:70): max_iter - 1 iterations.  rtol= / atol= are passed by like any keyword the reference does not '
                  'know; hs_pcg_stop takes them and stops on the device.')


def _make_hs_stop(name, preconditioned, where):
    single = name[:-len('_stop')]

    def run(A, b, x0, max_iter, preconditioner, callbacks, rtol, atol, kwargs):
        kwargs.pop('w_replace', None)
        if rtol is not None or atol is not None:
            kwargs.update(rtol=rtol, atol=atol)
        return _run(L.HS, name, A, b, x0, max_iter, preconditioner, callbacks, kwargs, hs_stop=True)
    if preconditioned:
        def f(A, b, x0, max_iter, preconditioner=None, callbacks=[], rtol=None, atol=None, **kwargs):
            return run(A, b, x0, max_iter, preconditioner, callbacks, rtol, atol, kwargs)
    else:
        def f(A, b, x0, max_iter, callbacks=[], rtol=None, atol=None, **kwargs):
            kwargs.pop('preconditioner', None)
            return run(A, b, x0, max_iter, None, callbacks, rtol, atol, kwargs)
    f.__doc__ = (f'{single} ({where}) in a session that can STOP by itself.  ' +
                 ('preconditioner: None, Jacobi(A) or a callable that is a diagonal scaling; anything else is a ValueError before the '
                  'device is reached.  ' if preconditioned else '') +
                 f'Without rtol= / atol= the result is {single}\'s, bit for bit.  rtol= and/or atol=: the session stops on the device once '
                 'its updated residual satisfies r.r <= max(rtol ||b||_2, atol)^2, or at a breakdown (prcg.h: prcg_set_stop_hs); the trial '
                 'dict then carries \'iterations\' and \'status\' (\'converged\' / \'breakdown\' / \'max_iter\'), histories are zero beyond '
                 f'the stop and callbacks are called up to the stop iteration and no further.  ({single} itself keeps passing rtol= / atol= by.)')
    f.__name__ = f.__qualname__ = name
    return f


hs_cg_stop = _make_hs_stop('hs_cg_stop', False, 'hs_cg.py:9')
hs_pcg_stop = _make_hs_stop('hs_pcg_stop', True, 'hs_cg.py:70')
pr_pcg = _make(L.PR, 'pr_pcg', True)                      # pr_cg.py:166
m_pcg = _make(L.M, 'm_pcg', True)                         # pr_cg.py:172
# the reference's unpreconditioned pr_cg / m_cg raise NameError (pr_cg.py:24,54); here
# they are the identity-preconditioned recurrences, which is what they were meant to be
pr_cg = _make(L.PR, 'pr_cg', False)
m_cg = _make(L.M, 'm_cg', False)
cg_cg = _make(L.CG_CG, 'cg_cg', False)                    # cg_cg.py:9   (Chronopoulos-Gear)
cg_pcg = _make(L.CG_CG, 'cg_pcg', True)                   # cg_cg.py:76
gv_cg = _make(L.GV, 'gv_cg', False)                       # gv_cg.py:9   (Ghysels-Vanroose, pipelined CG)
gv_pcg = _make(L.GV, 'gv_pcg', True)                      # gv_cg.py:93
pipe_p_cg = _make(L.PIPE_P, 'pipe_p_cg', False)           # pipe_pr_cg.py:83
pipe_pr_cg = _make(L.PIPE_PR, 'pipe_pr_cg', False)        # pipe_pr_cg.py:89
pipe_p_m_cg = _make(L.PIPE_P_M, 'pipe_p_m_cg', False)     # pipe_pr_cg.py:95
pipe_pr_m_cg = _make(L.PIPE_PR_M, 'pipe_pr_m_cg', False)  # pipe_pr_cg.py:101
pipe_p_pcg = _make(L.PIPE_P, 'pipe_p_pcg', True)          # pipe_pr_cg.py:195
pipe_pr_pcg = _make(L.PIPE_PR, 'pipe_pr_pcg', True)       # pipe_pr_cg.py:201
pipe_p_m_pcg = _make(L.PIPE_P_M, 'pipe_p_m_pcg', True)    # pipe_pr_cg.py:207
pipe_pr_m_pcg = _make(L.PIPE_PR_M, 'pipe_pr_m_pcg', True) # pipe_pr_cg.py:213
pipe_p_bpcg = _make_bpcg(L.PIPE_P, 'pipe_p_bpcg', 'pipe_pr_cg.py:195')
pipe_pr_bpcg = _make_bpcg(L.PIPE_PR, 'pipe_pr_bpcg', 'pipe_pr_cg.py:201')
pipe_p_m_bpcg = _make_bpcg(L.PIPE_P_M, 'pipe_p_m_bpcg', 'pipe_pr_cg.py:207')
pipe_pr_m_bpcg = _make_bpcg(L.PIPE_PR_M, 'pipe_pr_m_bpcg', 'pipe_pr_cg.py:213')

__all__ = ['hs_cg', 'hs_pcg', 'cg_cg', 'cg_pcg', 'gv_cg', 'gv_pcg', 'pr_cg', 'pr_pcg', 'm_cg', 'm_pcg',
           'pipe_p_cg', 'pipe_pr_cg', 'pipe_p_m_cg', 'pipe_pr_m_cg',
           'pipe_p_pcg', 'pipe_pr_pcg', 'pipe_p_m_pcg', 'pipe_pr_m_pcg', 'Jacobi', 'BlockJacobi',
           'hs_cg_multi', 'hs_pcg_multi', 'pr_cg_multi', 'pr_pcg_multi', 'm_cg_multi', 'm_pcg_multi',
           'pipe_pr_cg_multi', 'pipe_pr_pcg_multi', 'pipe_pr_m_cg_multi', 'pipe_pr_m_pcg_multi', 'clear_operator_cache', 'update_values',
           'pipe_pr_cg_batch', 'pipe_pr_m_cg_batch', 'hs_cg_batch', 'pipe_pr_pcg_batch', 'pipe_pr_m_pcg_batch', 'hs_pcg_batch',
           'pipe_pr_bpcg_batch', 'pipe_pr_m_bpcg_batch', 'hs_bpcg_batch', 'hs_bpcg_multi', 'pr_bpcg_multi', 'm_bpcg_multi',
           'invert_blocks', 'DeviceBlockJacobi', 'VarBlockJacobi', 'DeviceVarBlockJacobi',
           'pipe_p_bpcg', 'pipe_pr_bpcg', 'pipe_p_m_bpcg', 'pipe_pr_m_bpcg', 'hs_cg_stop', 'hs_pcg_stop']
