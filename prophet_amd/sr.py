"""Stochastic rounding of float32 to the two wire formats: the host definition.

``Compression.bf16_sr`` / ``fp16_sr`` round a float32 gradient up with a
probability equal to the fraction the 2-byte format drops, so the wire value
is right in expectation and no state is kept.  The result is a pure function
of ``(bits of g, key, step, element index)`` — there is no RNG state anywhere —
and the HIP kernels (``prophet_amd/csrc/bpsr_cast_sr.h``) are pinned bit for
bit to the numpy lines below.  Host tensors and numpy arrays go through them.

Random bits are Philox2x32-10 (Salmon et al., SC'11) with multiplier
``0xD256D193`` and key increment ``0x9E3779B9``: element ``i`` (0-based within
its tensor, whatever its address) takes 16 bits of
``philox2x32(c0 = i >> 2, c1 = step, k = key)``: the low and high half of
``x0`` for ``i & 3`` of 0 and 1, of ``x1`` for 2 and 3.  ``i >> 2`` is a
32-bit counter, so a tensor has at most 2^34 elements.

bf16, ``u`` the f32 bits: ``w = (u + r16) >> 16`` unless the exponent field is
all ones (inf stays inf, a NaN stays a NaN; the payload is not part of the
contract).  A value bf16 holds exactly is sent unchanged for every ``r16``;
f32 subnormals and signed zeros are kept; a finite value above bf16's largest
rounds to inf with the probability its position gives; over the 65,536 values
of ``r16`` the mean is exactly ``g``.

fp16: the value is cut to fp16 toward zero (``lo``), the dropped fraction is
taken to 16 bits (``f``) and ``h = lo + ((f + r16) >> 16)``, saturated at inf;
``|g| >= 65536`` is inf.  In the normal range ``f`` holds all 13 dropped bits
and the mean over ``r16`` is exact.  In fp16's subnormal range up to 39 bits
are dropped and ``f`` is their floor to 16, so the mean falls short of ``g`` by
at most 2^-16 of a subnormal step (2^-40): for ``1e-8`` it is ``9.99989e-9``.
"""
from __future__ import annotations

import numpy as np

PHILOX_M = 0xD256D193
PHILOX_W = 0x9E3779B9
MAX_ELEMS = 1 << 34           # i >> 2 is a 32-bit counter


def philox2x32(c0, c1, k):
    """Philox2x32-10 of counter ``(c0, c1)`` under key ``k`` (scalars or
    arrays, broadcast together): ``(x0, x1)`` as uint32 arrays."""
    c0, c1, k = np.broadcast_arrays(np.asarray(c0, np.uint64) & 0xffffffff,
                                    np.asarray(c1, np.uint64) & 0xffffffff,
                                    np.asarray(k, np.uint64) & 0xffffffff)
    m, w, mask = np.uint64(PHILOX_M), np.uint64(PHILOX_W), np.uint64(0xffffffff)
    s32 = np.uint64(32)
    for _ in range(10):
        prod = m * c0                      # 32 x 32 bits: fits 64
        c0, c1 = (prod >> s32) ^ k ^ c1, prod & mask
        k = (k + w) & mask                 # the bump after each round
    return c0.astype(np.uint32), c1.astype(np.uint32)


def sr_bits(n: int, key: int, step: int, first: int = 0):
    """The 16 random bits of elements ``first .. first + n - 1`` of a tensor
    under ``(key, step)``, as a uint32 array."""
    n, first = int(n), int(first)
    if first < 0 or n < 0 or first + n > MAX_ELEMS:
        raise ValueError(f"stochastic rounding of elements [{first}, {first + n}): "
                         f"at most {MAX_ELEMS} elements a tensor")
    if n == 0:
        return np.zeros(0, np.uint32)
    q0, q1 = first >> 2, (first + n - 1) >> 2
    x0, x1 = philox2x32(np.arange(q0, q1 + 1, dtype=np.uint64), int(step) & 0xffffffff,
                        int(key) & 0xffffffff)
    # a group's four draws in element order: x0 low, x0 high, x1 low, x1 high
    r = np.stack([x0 & np.uint32(0xffff), x0 >> np.uint32(16),
                  x1 & np.uint32(0xffff), x1 >> np.uint32(16)], axis=1).reshape(-1)
    return r[first - 4 * q0:first - 4 * q0 + n]


def _u32(g):
    g = np.ascontiguousarray(g)
    if g.dtype != np.float32:
        raise ValueError(f"stochastic rounding needs float32, got {g.dtype}")
    return g.reshape(-1).view(np.uint32)


def sr_bf16(g, r16):
    """bf16 bits (uint16) of float32 ``g`` under the 16-bit draws ``r16``."""
    u = _u32(g)
    r = np.asarray(r16, np.uint32) & np.uint32(0xffff)
    special = (u & np.uint32(0x7f800000)) == np.uint32(0x7f800000)
    # the plain compress there: inf as it is, a NaN quieted
    plain = (u >> np.uint32(16)) | np.where((u & np.uint32(0x7fffff)) != 0, 0x40, 0).astype(np.uint32)
    w = np.where(special, plain, (np.where(special, 0, u) + r) >> np.uint32(16))
    return w.astype(np.uint16)


def sr_fp16(g, r16):
    """fp16 bits (uint16) of float32 ``g`` under the 16-bit draws ``r16``."""
    u = _u32(g).astype(np.uint64)
    r = (np.asarray(r16, np.uint64) & np.uint64(0xffff))
    s = (u >> np.uint64(16)) & np.uint64(0x8000)
    a = u & np.uint64(0x7fffffff)
    e = a >> np.uint64(23)
    # normal fp16 range: 13 bits dropped, all of them in f
    lo_n = (a >> np.uint64(13)) - np.uint64(0x1c000)
    f_n = (a & np.uint64(0x1fff)) << np.uint64(3)
    # fp16 subnormals (and what is smaller): the significand shifted down
    m = (a & np.uint64(0x7fffff)) | np.where(e != 0, 0x800000, 0).astype(np.uint64)
    sh = np.uint64(126) - np.maximum(e, np.uint64(1))
    far = sh >= np.uint64(40)
    shc = np.where(far, 0, sh).astype(np.uint64)
    lo_s = np.where(far, 0, m >> shc).astype(np.uint64)
    f_s = np.where(far, 0, ((m << np.uint64(16)) >> shc) & np.uint64(0xffff)).astype(np.uint64)
    normal = e >= np.uint64(113)
    lo = np.where(normal, lo_n, lo_s)
    f = np.where(normal, f_n, f_s)
    h = np.minimum(lo + ((f + r) >> np.uint64(16)), np.uint64(0x7c00))
    h = np.where(a >= np.uint64(0x47800000), np.uint64(0x7c00), h)
    # the plain compress for inf and NaN
    h = np.where(e == np.uint64(0xff),
                 np.where(a > np.uint64(0x7f800000), 0x7e00, 0x7c00).astype(np.uint64), h)
    return (s | h).astype(np.uint16)


def sr_round(g, key: int, step: int, wire: str, first: int = 0):
    """``sr_bf16`` / ``sr_fp16`` (``wire``: "bf16" or "fp16") of a whole
    tensor whose first element has index ``first``."""
    u = _u32(g)
    r = sr_bits(u.size, key, step, first)
    return (sr_bf16 if wire == "bf16" else sr_fp16)(u.view(np.float32), r)


def context_key(declared_key: int, rank: int, seed: int) -> int:
    """The key a worker's context rounds under: ``x0`` of
    ``philox2x32(c0 = declared key, c1 = rank, k = seed)`` — ranks draw
    independent bits, so their rounding errors do not add coherently."""
    x0, _ = philox2x32(int(declared_key) & 0xffffffff, int(rank) & 0xffffffff,
                       int(seed) & 0xffffffff)
    return int(x0)


__all__ = ["philox2x32", "sr_bits", "sr_bf16", "sr_fp16", "sr_round", "context_key",
           "PHILOX_M", "PHILOX_W", "MAX_ELEMS"]
