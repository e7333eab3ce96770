"""Stateless block-scaled 8- and 4-bit wires: stochastic rounding, and an
optional random-sign Hadamard rotation of every block.  The host definition.

``Compression.mxfp8_sr`` / ``mxfp4_sr`` are ``mx.py``'s wire without its
residual: a code is rounded up with a probability equal to the fraction the
format drops, under the 16 bits ``fp16_sr`` gives the element
(``sr.sr_bits(n, key, step)``), so the decode is right in expectation and no
state is kept.  ``mxfp8_rht_sr`` / ``mxfp4_rht_sr`` rotate every whole block of
32 first, which spreads a block's largest element over all of them (at 4 bits
plain stochastic rounding has a variance set by that element); the rotation is
linear, so it is undone once, after the sum.  The HIP kernels
(``prophet_amd/csrc/bpsr_k_mx_sr.hip``, ``byteps_reduce_mx_sr_*`` and
``byteps_reduce_mx_rht_fold_*``) are pinned to the numpy lines below, byte for
byte; host tensors and numpy arrays go through them.

The payload is ``mx.py``'s (``mx.payload_bytes``); the header's fourth u32 is 1
for a rotated payload.  With ``emax`` 8 / 2, ``max`` 448 / 6, ``mbits`` 3 / 1,
``emin`` -6 / 0 and ``MANT`` 0x600000 / 0x400000 for fp8 / fp4::

    c     = g                                   unrotated
            H (D_b g)                           rotated, whole blocks only (below)
    K_b   = max over the block of bits(c_i) & 0x7fffffff;  E_b = K_b >> 23
    X_b   = 255                                 if E_b == 255
            max(E_b - emax + bump, 0)           bump = (K_b & 0x7fffff) > MANT
    v_i   = c_i * 2^(127 - X_b)                 one float32 multiply
    s     = max(floor(log2 |v_i|), emin) - mbits
    k, f  = floor(|v_i| / 2^s), floor(frac(|v_i| / 2^s) * 2^16)
    code  = the format's code of (k + ((f + r16_i) >> 16)) * 2^s, v_i's sign kept

The bump is the one difference from ``mx.py``'s scale: it keeps ``|v_i| <=
max``, so nothing is clamped and the wire is unbiased.  On the bits ``a`` of
``|v_i|`` the rounding is a shift and an add (``sr_encode``): the codes of a
format ascend with the magnitude, so a carry runs into the exponent by itself.
A block with ``X_b == 255`` (an inf or a NaN) carries codes of 0.

Rotation.  Block ``b`` takes the sign word ``w_b = x0 of philox2x32(c0 = b, c1
= step, k = rot_key)``; element ``32 b + j`` has its sign bit flipped (an xor)
when bit ``j`` of ``w_b`` is set, and the block then goes through the
unnormalised Walsh-Hadamard butterflies in a fixed order — for ``h`` in 1, 2,
4, 8, 16 every pair ``(i, i + h)`` with ``i & h == 0`` becomes ``(a + b, a -
b)``, each one IEEE float32 operation.  A last block of fewer than 32 elements
has no room on the wire for the coefficients its padding would take: it is not
rotated, in the compress or in the fold.  Every worker of a tensor shares
``rot_key`` (``rotation_key``); the rounding ``key`` differs by rank.

``decode`` is ``mx.decode``.  The unrotated fold is ``mx.fold``.  The rotated
fold: ``t`` the float32 left fold of the decodes, ``z`` the butterflies of
``t``, ``out_i = z_i * 2^-5`` with the sign flipped by bit ``j`` of ``w_b``,
then one divide by ``f32(divisor)`` above 1.  A block where any source has
``X_b == 255`` is ``0x7fc00000`` in every element.  Where finite decodes
overflow inside the sum or the butterflies only "not finite" is contracted.

A float16 or bf16 gradient is widened exactly to float32 first, and a fold into
a float16 or bf16 output converts the float32 result once (``mx.widen``,
``mx.narrow``).
"""
from __future__ import annotations

import numpy as np

from . import mx, sr

# fmt: the largest mantissa field of K_b that 2^emax still holds at or below max
_MANT = {"fp8": 0x600000, "fp4": 0x400000}
_NAN = np.uint32(0x7fc00000)


def rotation_key(declared_key: int, seed: int) -> int:
    """The rotation key every worker of a tensor shares: ``x1`` of the Philox
    call ``sr.context_key`` makes at rank 0."""
    _, x1 = sr.philox2x32(int(declared_key) & 0xffffffff, 0, int(seed) & 0xffffffff)
    return int(x1)


def sign_words(nblocks: int, rot_key: int, step: int):
    """``w_b`` of blocks ``0 .. nblocks - 1`` (uint32)."""
    if int(nblocks) == 0:
        return np.zeros(0, np.uint32)
    x0, _ = sr.philox2x32(np.arange(int(nblocks), dtype=np.uint64), int(step) & 0xffffffff,
                          int(rot_key) & 0xffffffff)
    return x0


def _sign_masks(nblocks: int, rot_key: int, step: int):
    """Rows of 32 uint32: ``0x80000000`` where the block's word has the bit."""
    w = sign_words(nblocks, rot_key, step)[:, None]
    return ((w >> np.arange(32, dtype=np.uint32)) & np.uint32(1)) << np.uint32(31)


def butterflies(blocks):
    """The unnormalised Walsh-Hadamard transform of rows of 32 float32."""
    x = np.array(blocks, dtype=np.float32).reshape(-1, 32)
    i = np.arange(32)
    with np.errstate(all="ignore"):
        for h in (1, 2, 4, 8, 16):
            lo = i[(i & h) == 0]
            a, b = x[:, lo].copy(), x[:, lo + h].copy()
            x[:, lo], x[:, lo + h] = a + b, a - b
    return x


def _whole(n: int, nblocks: int):
    """Which blocks are rotated: all but a last one of fewer than 32 elements."""
    whole = np.ones(nblocks, dtype=bool)
    if int(n) % mx.BLOCK:
        whole[-1] = False
    return whole


def rotate(g, rot_key: int, step: int):
    """``c`` of the rotated wire, as rows of 32 (the last row padded with +0.0
    and, where it is padded, left as it is)."""
    g = mx._f32(g)
    blocks = mx._blocks(g)
    flipped = (blocks.view(np.uint32) ^ _sign_masks(blocks.shape[0], rot_key, step)) \
        .view(np.float32)
    return np.where(_whole(g.size, blocks.shape[0])[:, None], butterflies(flipped), blocks)


def scales(blocks, fmt):
    """``X_b`` (uint8) of rows of 32 float32."""
    emax = mx._fmt(fmt)[1]
    key = np.ascontiguousarray(blocks, np.float32).reshape(-1, 32).view(np.uint32) \
        & np.uint32(0x7fffffff)
    k = key.max(axis=1, initial=0).astype(np.int64)
    e = k >> 23
    bump = ((k & 0x7fffff) > _MANT[fmt]).astype(np.int64)
    return np.where(e == 255, 255, np.maximum(e - emax + bump, 0)).astype(np.uint8)


def sr_encode(v, r16, fmt):
    """The codes (uint8) of float32 ``v``, ``|v| <= max``, under the 16-bit
    draws ``r16``."""
    bits, _, _, mbits, bias = mx._fmt(fmt)
    v = mx._f32(v)
    r = np.asarray(r16, np.uint64) & np.uint64(0xffff)
    a = (v.view(np.uint32) & np.uint32(0x7fffffff)).astype(np.uint64)
    e = a >> np.uint64(23)
    drop = np.uint64(23 - mbits)
    # normals of the format: mbits of the mantissa stay, the next 16 are f
    lo_n = (a >> drop).astype(np.int64) - ((127 - bias) << mbits)
    f_n = (a >> (drop - np.uint64(16))) & np.uint64(0xffff)
    # below 2^emin: the significand shifted down to multiples of 2^(emin - mbits)
    m = (a & np.uint64(0x7fffff)) | np.where(e != 0, 0x800000, 0).astype(np.uint64)
    sh = np.uint64(150 + 1 - bias - mbits) - np.maximum(e, np.uint64(1))
    far = sh >= np.uint64(40)
    shc = np.where(far, 0, sh).astype(np.uint64)
    lo_s = np.where(far, 0, m >> shc).astype(np.int64)
    f_s = np.where(far, 0, ((m << np.uint64(16)) >> shc) & np.uint64(0xffff)).astype(np.uint64)
    normal = e >= np.uint64(128 - bias)
    lo = np.where(normal, lo_n, lo_s)
    f = np.where(normal, f_n, f_s)
    code = lo + ((f + r) >> np.uint64(16)).astype(np.int64)
    sign = (v.view(np.uint32) >> np.uint32(31)).astype(np.int64) << (bits - 1)
    return (code | sign).astype(np.uint8)


def quantise(blocks, r16, fmt):
    """``(X uint8 [blocks], q uint8 [32 blocks])`` of rows of 32 float32 under
    the draws ``r16`` (one an element, padding included)."""
    c = np.ascontiguousarray(blocks, np.float32).reshape(-1)
    x = scales(c, fmt)
    xe = np.repeat(x, mx.BLOCK).astype(np.int64)
    bad = xe == 255
    with np.errstate(all="ignore"):
        v = (c * mx._pow2(np.where(bad, 127, 254 - xe))).astype(np.float32)
    v = np.where(bad, np.float32(0.0), v)
    return x, np.where(bad, 0, sr_encode(v, r16, fmt)).astype(np.uint8)


def compress(g, fmt, key: int, step: int, rotate_blocks: bool = False, rot_key: int = 0,
             bf16: bool = False):
    """The payload (a new uint8 array) of the gradient ``g``: float32, float16,
    or with ``bf16`` its bf16 bits, widened exactly first (``mx.widen``)."""
    g = mx.widen(g, bf16)
    if g.size > mx.MAX_ELEMS:
        raise ValueError("mx_sr: more than 2^31 elements")
    n, bits = g.size, mx.bits_of(fmt)
    blocks = rotate(g, rot_key, step) if rotate_blocks else mx._blocks(g)
    r16 = np.zeros(blocks.size, np.uint32)
    r16[:n] = sr.sr_bits(n, key, step)
    x, q = quantise(blocks, r16, fmt)
    q = q[:n]
    payload = np.zeros(mx.payload_bytes(n, fmt), dtype=np.uint8)
    payload[0:4] = np.array([bits], dtype="<u4").view(np.uint8)
    payload[4:12] = np.array([n], dtype="<u8").view(np.uint8)
    payload[12:16] = np.array([1 if rotate_blocks else 0], dtype="<u4").view(np.uint8)
    at = mx.HEADER_BYTES
    payload[at:at + x.size] = x
    at += mx._align16(x.size)
    if bits == 4:
        pairs = np.zeros(2 * mx.code_bytes(n, fmt), dtype=np.uint8)
        pairs[:n] = q
        q = pairs[0::2] | (pairs[1::2] << 4)
    payload[at:at + q.size] = q
    return payload


def rotated(payload) -> bool:
    """The header's flag (never used for sizes)."""
    p = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
    return bool(p[12:16].view("<u4")[0])


def fold(payloads, n: int, fmt, divisor: int = 1, rotate_blocks: bool = False,
         rot_key: int = 0, step: int = 0, out_dtype=None):
    """The N-way decode of payloads compressed under one ``rotate_blocks``,
    ``rot_key`` and ``step``: a new array of ``n`` elements, the float32
    result converted once to ``out_dtype`` (``mx.narrow``)."""
    if not rotate_blocks:
        return mx.fold(payloads, n, fmt, divisor, out_dtype)
    n = int(n)
    out = mx.fold(payloads, n, fmt, 1)            # t, and the checks
    t = mx._blocks(out)
    whole = _whole(n, t.shape[0])
    bad = np.zeros(t.shape[0], dtype=bool)
    for p in payloads:
        bad |= mx.fields(p, n, fmt)[0] == 255
    with np.errstate(all="ignore"):
        z = butterflies(t) * np.float32(2.0 ** -5)
        z = (z.view(np.uint32) ^ _sign_masks(t.shape[0], rot_key, step)).view(np.float32)
        z = np.where(whole[:, None], z, t)
        if int(divisor) > 1:
            z = z / np.float32(int(divisor))
    z = np.where(bad[:, None], _NAN.view(np.float32), z).astype(np.float32)
    return mx.narrow(z.reshape(-1)[:n].copy(), out_dtype)


__all__ = ["rotation_key", "sign_words", "butterflies", "rotate", "scales", "sr_encode",
           "quantise", "compress", "rotated", "fold"]
