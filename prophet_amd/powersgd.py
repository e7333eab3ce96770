"""PowerSGD low-rank compression with error feedback: the host definition and
the round.

A float32 tensor of shape ``(d0, d1, ...)`` is the matrix ``M`` with ``n = d0``
rows and ``m = prod(d1...)`` columns.  With a rank ``r``, 1..16, it travels as
``P`` (n x r) and ``Q`` (m x r), plain float32 matrices the PS server's fp32
fold sums as it sums any tensor: ``(n + m) r`` floats in place of ``n m``.
``compresses(t, r)`` is the shape rule; everything else passes through.

The state per tensor (:class:`State`) is the float32 residual ``R`` (n x m,
zero at start) and the warm start ``Q`` (m x r, ``init_q``: drawn once from a
seeded ``default_rng``, the same on every worker).  One iteration, the caller
averaging ``P`` after the first line and ``Qn`` after the third::

    project_p(g, R, Q):   R[:] = g + R            # one f32 add; R now holds M
                          P = R @ Q               # n x r
    orthogonalize(P):     modified Gram-Schmidt over columns 0..r-1, in place;
                          dot products and squared norms accumulated in float64;
                          a column whose squared norm is 0 or non-finite becomes zeros
    project_q(R, P):      Qn = R.T @ P            # m x r, R still holds M
    finish(out, R, P, Q): a = 0; for k in 0..r-1: a = a + P[:, k:k+1] * Q[None, :, k]
                          out[:] = a;  R[:] = where(isfinite(a) & isfinite(R), R - a, 0)

``finish`` takes the aggregated ``Qn``, which is the next iteration's warm
start.  Every function takes ``dtype=``: the same lines in float64 are the
reference the tests hold the float32 paths to.

This is the first wire whose device path (``byteps_reduce_powersgd_*``,
``prophet_amd/csrc/bpsr_k_powersgd.hip``) is NOT pinned to these lines byte for
byte throughout.  The two contractions over thousands of terms, ``R @ Q`` and
``R.T @ P``, run on f32 matrix instructions in an order that belongs to the
kernels (numpy's own order belongs to its BLAS); they are held to the error
bound of an f32 dot product, ``gamma_K (|M| @ |Q|)``.  ``orthogonalize`` sums in
float64 in the kernel's order.  Pinned byte for byte: the ``g + R`` written
into ``R``; all of ``finish`` given its inputs; and determinism — the same plan
on the same bytes gives the same bytes, there are no float atomics.

``push_pull_many`` is the round over a :class:`~prophet_amd.pushpull.Worker`.
"""
from __future__ import annotations

import numpy as np

MAX_RANK = 16


def shape_of(t) -> tuple:
    """``(n, m)`` of a tensor or array of two or more dimensions."""
    shape = tuple(int(d) for d in t.shape)
    return shape[0], int(np.prod(shape[1:], dtype=np.int64))


def _is_f32(t) -> bool:
    return str(t.dtype).rsplit(".", 1)[-1] == "float32"


def compresses(t, r: int) -> bool:
    """float32, two or more dimensions, and fewer floats on the wire than in
    the tensor: ``(n + m) r < n m``."""
    if not 1 <= int(r) <= MAX_RANK:
        raise ValueError(f"rank {r} outside 1..{MAX_RANK}")
    if not _is_f32(t) or len(t.shape) < 2:
        return False
    n, m = shape_of(t)
    return (n + m) * int(r) < n * m


def init_q(m: int, r: int, seed: int, dtype=np.float32):
    """The warm start: standard normals from ``default_rng(seed)``."""
    return np.random.default_rng(int(seed)).standard_normal((int(m), int(r))).astype(dtype)


def _own(x, dtype, what):
    if not isinstance(x, np.ndarray) or x.dtype != dtype or x.ndim != 2:
        raise ValueError(f"{what} must be a 2-d {np.dtype(dtype).name} array written in place")
    return x


def project_p(g, R, Q, dtype=np.float32):
    R = _own(R, dtype, "R")
    R[:] = np.asarray(g, dtype).reshape(R.shape) + R
    return R @ np.asarray(Q, dtype)


def orthogonalize(P, dtype=np.float32):
    P = _own(P, dtype, "P")
    f64 = np.float64
    with np.errstate(invalid="ignore", over="ignore"):        # a non-finite column is dropped
        for k in range(P.shape[1]):
            for j in range(k):
                d = np.dot(P[:, j].astype(f64), P[:, k].astype(f64))
                P[:, k] = (P[:, k].astype(f64) - d * P[:, j].astype(f64)).astype(dtype)
            s = np.dot(P[:, k].astype(f64), P[:, k].astype(f64))
            if s > 0 and np.isfinite(s):
                P[:, k] = (P[:, k].astype(f64) / np.sqrt(s)).astype(dtype)
            else:
                P[:, k] = 0
    return P


def project_q(R, P, dtype=np.float32):
    return np.asarray(R, dtype).T @ np.asarray(P, dtype)


def finish(out, R, P, Q, dtype=np.float32):
    R = _own(R, dtype, "R")
    P, Q = np.asarray(P, dtype), np.asarray(Q, dtype)
    a = np.zeros(R.shape, dtype)
    for k in range(P.shape[1]):
        a = a + P[:, k:k + 1] * Q[None, :, k]
    out.reshape(R.shape)[:] = a
    with np.errstate(invalid="ignore"):
        R[:] = np.where(np.isfinite(a) & np.isfinite(R), R - a, 0)
    return out


class State:
    """One tensor's PowerSGD state: the residual ``R`` (n x m), the warm start
    ``Q`` and the wire buffers ``P`` (n x r) and ``Qn`` (m x r), all float32
    and of the tensor's kind and device.  After ``finish`` the aggregated
    ``Qn`` is the warm start: the two buffers change places."""

    __slots__ = ("rank", "n", "m", "R", "Q", "P", "Qn")

    def __init__(self, rank, n, m, R, Q, P, Qn):
        self.rank, self.n, self.m = int(rank), int(n), int(m)
        self.R, self.Q, self.P, self.Qn = R, Q, P, Qn


def make_states(named_grads, rank: int, seed: int = 0) -> dict:
    """A :class:`State` per tensor that compresses (None for the others), the
    i-th tensor's warm start drawn under ``seed + i``."""
    from .compression import Compression
    return {name: Compression.powersgd_ef.state_like(t, rank, int(seed) + i)
            for i, (name, t) in enumerate(named_grads.items())}


def _dtype_id(t) -> int:
    from .dtypes import DType, from_torch, numpy_dtype
    if hasattr(t, "data_ptr"):
        return int(from_torch(t.dtype))
    return int(next(d for d in DType if d != DType.BFLOAT16 and numpy_dtype(d) == t.dtype))


def push_pull_many(worker, named_grads, states, average: bool = True, plans=None):
    """One PowerSGD round over ``worker`` for the gradients ``named_grads``
    (name -> tensor, the same names in the same order on every worker), in
    place.  ``states``: ``make_states``'.  ``name + ".P"`` and ``name + ".Q"`` are
    declared as ordinary float32 tensors with ``Compression.none`` on first use.
    ``project_p``, one ``push_pull_iteration`` over every ``P`` and every tensor
    that does not compress (it travels as it is), ``orthogonalize``,
    ``project_q``, one iteration over every ``Qn``, ``finish`` into the
    gradients.  ``plans``: a ``CastPlanCache`` that keeps the device plans."""
    from .compression import Compression
    from .dtypes import DType
    C = Compression.powersgd_ef
    comp = [nm for nm in named_grads if states.get(nm) is not None]
    first, second = {}, {}
    for nm, g in named_grads.items():
        st = states.get(nm)
        wire = [(nm, g, _dtype_id(g), first)] if st is None else \
            [(nm + ".P", st.P, DType.FLOAT32, first), (nm + ".Q", st.Qn, DType.FLOAT32, second)]
        for key, buf, dtype, it in wire:
            ctx = worker.contexts.get(key)
            if ctx is None or not ctx.initialized:
                worker.init_tensor(key, buf, dtype, compression=Compression.none)
            it[key] = buf
    grads, sts = [named_grads[nm] for nm in comp], [states[nm] for nm in comp]
    C.project_p_many(grads, sts, plans)
    if first:
        worker.push_pull_iteration(first, average=average)
    C.orthogonalize_many(grads, sts, plans)
    C.project_q_many(grads, sts, plans)
    if second:
        worker.push_pull_iteration(second, average=average)
    C.finish_many(grads, sts, plans)
    return named_grads


__all__ = ["MAX_RANK", "shape_of", "compresses", "init_q", "project_p", "orthogonalize",
           "project_q", "finish", "State", "make_states", "push_pull_many"]
