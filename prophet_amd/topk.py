"""Top-k sparsification with error feedback: the host definition.

BytePS's sparsifier (Deep Gradient Compression): a tensor travels as its ``k``
values of largest magnitude with their indices, and a per-tensor float32
residual ``r`` keeps the rest for the next step.  The HIP kernels
(``prophet_amd/csrc/bpsr_k_topk.hip``, ``byteps_reduce_topk_*``) are pinned to
the numpy lines below, byte for byte; host tensors and numpy arrays go through
them.  For ``n`` float32 elements ``g`` and ``1 <= k <= n``::

    c_i   = g_i + r_i                  one IEEE float32 add
    key_i = bits(c_i) & 0x7fffffff     uint32: orders |c|, NaN above inf, -0.0 == +0.0
    T     = the k-th largest key
    sel   = every i with key_i > T, and of those with key_i == T the first
            (k - #{key > T}) in ascending i: exactly k elements
    r'_i  = +0.0 if i in sel else c_i
    payload values = the bits of c_i for i in sel, ascending i

The payload, little endian, ``16 + 8 k`` bytes: the header ``{u32 k, u32 n_lo,
u32 n_hi, u32 0}``, then ``k`` uint32 indices, strictly ascending, then ``k``
float32 values.  ``n == 0`` means ``k == 0`` and a bare header.

``decode(payload, n, k)`` is zeros with ``out[idx] = val``.  ``fold`` starts
from +0.0 and runs over the sources in argument order, ``out[idx_s] =
out[idx_s] + val_s`` (one float32 add each), then one divide by
``f32(divisor)`` when ``divisor > 1``.  Sizes come from the caller (``k`` from
the payload's byte count when not given): a header is never trusted.  There is
no floating-point reduction anywhere in the scheme, so every byte is pinned.

``refold(payloads, n, r, k)`` is the server round: ``compress(fold(payloads, n,
1, k), r, k)`` against the server's own residual — nothing new is defined.
"""
from __future__ import annotations

import math

import numpy as np

HEADER_BYTES = 16
MAX_SRCS = 16
MAX_ELEMS = 1 << 31
# the fourth header word of a key's init payload ("topk"): how the packed-round
# store tells a top-k key from the wires whose first header word names them
INIT_TAG = 0x6b706f74


def payload_bytes(k: int) -> int:
    """Bytes of a payload of ``k`` entries."""
    if int(k) < 0:
        raise ValueError(f"negative entry count {k}")
    return HEADER_BYTES + 8 * int(k)


def k_for(n: int, ratio: float) -> int:
    """``min(n, max(1, ceil(n * ratio)))`` (0 for an empty tensor)."""
    n = int(n)
    if n < 0 or not ratio > 0:
        raise ValueError(f"k_for({n}, {ratio})")
    return min(n, max(1, math.ceil(n * ratio)))


def k_of(payload) -> int:
    """``k`` of a payload buffer, from its size: ``(bytes - 16) / 8``."""
    size = int(payload.numel()) if hasattr(payload, "numel") else int(payload.size)
    if size < HEADER_BYTES or (size - HEADER_BYTES) % 8:
        raise ValueError(f"topk: no payload has {size} bytes")
    return (size - HEADER_BYTES) // 8


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32).reshape(-1)


def keys(c):
    """``bits(c) & 0x7fffffff`` of a float32 array."""
    return _f32(c).view(np.uint32) & np.uint32(0x7fffffff)


def select(c, k: int):
    """``sel`` as ascending indices (int64) of the float32 array ``c``."""
    key = keys(c)
    n, k = key.size, int(k)
    if not (1 <= k <= n or n == k == 0):
        raise ValueError(f"topk: k {k} outside 1..{n}")
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    t = np.partition(key, n - k)[n - k]
    gt = np.flatnonzero(key > t)
    eq = np.flatnonzero(key == t)[:k - gt.size]
    return np.sort(np.concatenate([gt, eq]))


def compress(g, r, k: int):
    """One step: ``(payload, r')`` — the payload as a new uint8 array, the new
    residual as a new float32 array — from the float32 arrays ``g`` and ``r``."""
    g, r = _f32(g), _f32(r)
    if g.size != r.size:
        raise ValueError(f"topk: {g.size} elements, {r.size} residuals")
    if g.size > MAX_ELEMS:
        raise ValueError("topk: more than 2^31 elements")
    with np.errstate(all="ignore"):
        c = g + r
    sel = select(c, k)
    payload = np.zeros(payload_bytes(sel.size), dtype=np.uint8)
    payload[0:4] = np.array([sel.size], dtype="<u4").view(np.uint8)
    payload[4:12] = np.array([g.size], dtype="<u8").view(np.uint8)
    payload[HEADER_BYTES:HEADER_BYTES + 4 * sel.size] = sel.astype("<u4").view(np.uint8)
    payload[HEADER_BYTES + 4 * sel.size:] = c[sel].astype("<f4").view(np.uint8)
    rn = c.copy()
    rn[sel] = np.float32(0.0)
    return payload, rn


def header(payload):
    """``(k, n)`` as a payload's header states them (never used for sizes)."""
    p = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
    return int(p[0:4].view("<u4")[0]), int(p[4:12].view("<u8")[0])


def entries(payload, k: int | None = None):
    """``(indices uint32, values float32)`` of a payload of ``k`` entries."""
    p = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
    k = k_of(p) if k is None else int(k)
    if p.size < payload_bytes(k):
        raise ValueError(f"topk: a {p.size}-byte payload for {k} entries")
    idx = p[HEADER_BYTES:HEADER_BYTES + 4 * k].view("<u4")
    val = p[HEADER_BYTES + 4 * k:HEADER_BYTES + 8 * k].view("<f4")
    return idx, val


def decode(payload, n: int, k: int | None = None):
    """Zeros with ``out[idx] = val``: a new float32 array of ``n`` elements.
    (The one-source ``fold`` adds to +0.0 instead: a value of -0.0 arrives as
    +0.0 there, every other value the same.)"""
    idx, val = entries(payload, k)
    out = np.zeros(int(n), dtype=np.float32)
    ok = idx < n
    out[idx[ok].astype(np.int64)] = val[ok]
    return out


def fold(payloads, n: int, divisor: int = 1, k: int | None = None):
    """The N-way decode-and-sum.  An index outside ``[0, n)`` (a malformed
    payload) is dropped."""
    if not 1 <= len(payloads) <= MAX_SRCS:
        raise ValueError(f"topk: {len(payloads)} sources outside 1..{MAX_SRCS}")
    if int(divisor) < 1:
        raise ValueError(f"divisor {divisor} < 1")
    out = np.zeros(int(n), dtype=np.float32)
    with np.errstate(all="ignore"):
        for p in payloads:
            idx, val = entries(p, k)
            ok = idx < n
            idx = idx[ok].astype(np.int64)
            out[idx] = out[idx] + val[ok]
        if int(divisor) > 1:
            out = out / np.float32(int(divisor))
    return out.astype(np.float32)


def refold(payloads, n: int, resid, k: int | None = None):
    """The server round: ``compress(fold(payloads, n, 1,
    k), resid, k)`` — ``(payload, r')`` as new arrays.  1..16 payloads of the
    same ``k`` (from their byte count when not given), folded left in argument
    order from +0.0; the server does not divide."""
    if k is None:
        k = k_of(np.ascontiguousarray(payloads[0]).reshape(-1).view(np.uint8)) if payloads else 0
    return compress(fold(payloads, n, 1, k), resid, k)


def init_payload(n: int, k: int):
    """What a key's init push carries (``packed_round.PackedRound``): the
    compress of ``n`` zeros — indices 0..k-1, values +0.0 — with ``INIT_TAG``
    in the fourth header word, which every other wire's init header, and every
    payload a kernel reads or writes, leaves zero.  It is never folded."""
    z = np.zeros(int(n), dtype=np.float32)
    payload, _ = compress(z, z, int(k))
    payload[12:16] = np.array([INIT_TAG], dtype="<u4").view(np.uint8)
    return payload


__all__ = ["HEADER_BYTES", "MAX_SRCS", "MAX_ELEMS", "INIT_TAG", "payload_bytes", "k_for", "k_of",
           "keys", "select", "compress", "header", "entries", "decode", "fold", "refold",
           "init_payload"]
