"""Block-scaled 8- and 4-bit gradient wires with error feedback: the host
definition.

Every 32 consecutive elements (by index in the tensor; the last block padded
with +0.0) share one power-of-two scale, an E8M0 byte, and travel as OCP
``e4m3`` (``fmt="fp8"``, the ``fn`` encoding of ``torch.float8_e4m3fn``) or OCP
``e2m1`` (``fmt="fp4"``) codes: 8.25 or 4.25 bits an element.  A per-tensor
float32 residual ``r`` keeps what the wire dropped.  The HIP kernels
(``prophet_amd/csrc/bpsr_k_mx.hip``, ``byteps_reduce_mx_*``) are pinned to the
numpy lines below, byte for byte; host tensors and numpy arrays go through
them.  With ``emax`` 8 / 2 and ``max`` 448 / 6 for fp8 / fp4::

    c_i   = g_i + r_i                                  one IEEE float32 add
    key_i = bits(c_i) & 0x7fffffff                     uint32
    E_b   = (max over the block of key_i) >> 23        an integer maximum
    X_b   = 255                       if E_b == 255    (an inf or NaN in the block)
            clamp(E_b - emax, 0, 254) otherwise        the scale byte, 2^(X_b - 127)
    v_i   = clamp(c_i * 2^(127 - X_b), -max, +max)     one float32 multiply, then saturate
    q_i   = v_i rounded to the format, nearest, ties to even, the sign kept
    d_i   = f32(q_i) * 2^(X_b - 127)                   one float32 multiply, exact
    r'_i  = c_i - d_i                                  one IEEE float32 subtract

A block with ``X_b == 255`` carries codes of 0 and decodes to the NaN
``0x7fc00000`` in every element; its ``r'_i`` is that NaN too, in these bits
(what ``c_i - NaN`` gives differs between machines in the sign and the
payload).  ``2^(127 - X)`` is the float32 ``(254 - X) << 23``; ``2^(X - 127)``
is ``X << 23``, and the subnormal ``0x00400000`` for ``X == 0``.

The payload, little endian: the header ``{u32 bits (8 or 4), u32 n_lo, u32
n_hi, u32 0}``, ``ceil(n / 32)`` scale bytes padded with zeros to a multiple of
16, then the codes padded with zeros to a multiple of 16 — ``n`` bytes (fp8) or
``ceil(n / 2)`` bytes with element ``2 j`` in the low nibble (fp4).

``decode(payload, n, fmt)`` gives ``d``.  ``fold`` is the float32 left fold of
the decodes in argument order, then one divide by ``f32(divisor)`` when
``divisor > 1``.  Sizes come from the caller: a header is never trusted.  There
is no floating-point reduction anywhere in the scheme, so every byte is pinned.
``refold`` is the server round: the ``compress`` of that
fold, undivided, against the server's own residual.

Half-precision tensors (DESIGN.md §11.16;
``prophet_amd/csrc/bpsr_k_mx_half.hip``).  A float16 or bf16 gradient is
widened exactly to float32 (``widen``) and the lines above run on that: its
payload is the payload of its upcast, and ``r`` stays float32.  A fold into a
float16 or bf16 output computes the float32 result above and converts it once
(``narrow``).
"""
from __future__ import annotations

import numpy as np

HEADER_BYTES = 16
BLOCK = 32
MAX_SRCS = 16
MAX_ELEMS = 1 << 31

# fmt: (bits, emax, max, mantissa bits, exponent bias)
_FORMATS = {"fp8": (8, 8, 448.0, 3, 7), "fp4": (4, 2, 6.0, 1, 1)}


def _fmt(fmt):
    try:
        return _FORMATS[fmt]
    except (KeyError, TypeError):
        raise ValueError(f"mx: unknown format {fmt!r} (fp8, fp4)") from None


def bits_of(fmt) -> int:
    """Bits an element code: 8 or 4."""
    return _fmt(fmt)[0]


def _align16(x: int) -> int:
    return (x + 15) & ~15


def scale_bytes(n: int) -> int:
    """``ceil(n / 32)``: the blocks, one scale byte each."""
    return (int(n) + BLOCK - 1) // BLOCK


def code_bytes(n: int, fmt) -> int:
    """``ceil(n * bits / 8)``."""
    return (int(n) * bits_of(fmt) + 7) // 8


def payload_bytes(n: int, fmt) -> int:
    """Bytes of the payload of ``n`` elements."""
    if int(n) < 0:
        raise ValueError(f"negative element count {n}")
    return HEADER_BYTES + _align16(scale_bytes(n)) + _align16(code_bytes(n, fmt))


def _f32(x):
    return np.ascontiguousarray(x, dtype=np.float32).reshape(-1)


def widen(g, bf16: bool = False):
    """The gradient as a flat float32 array, exactly: a float16 array is
    widened, ``bf16`` says ``g`` holds bf16 bits (uint16), float32 is itself."""
    if bf16:
        bits = np.ascontiguousarray(g).reshape(-1).view(np.uint16)
        return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    return _f32(g)


def narrow(x, out_dtype=None):
    """The float32 array ``x`` in a fold's output type, converted once:
    ``None`` or ``"float32"`` as it is; ``"float16"`` a float16 array;
    ``"bfloat16"`` bf16 bits (uint16).  Nearest, ties to even, overflow to
    infinity, subnormals kept; a NaN as the f32 -> fp16 / bf16 casts of
    ``Compression.fp16`` / ``bf16`` make it (``f2h_bits``, ``f32_to_bf16_rne``
    of ``prophet_amd/csrc/bpsr_ops.h``): the sign, quiet, the payload's top
    bits."""
    x = _f32(x)
    if out_dtype in (None, "float32"):
        return x
    u = x.view(np.uint32)
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    if out_dtype == "float16":
        with np.errstate(all="ignore"):
            h = x.astype(np.float16).view(np.uint16)
        as_nan = ((u >> np.uint32(16)) & np.uint32(0x8000)) | np.uint32(0x7e00) \
            | ((u >> np.uint32(13)) & np.uint32(0x3ff))
        return np.where(nan, as_nan, h).astype(np.uint16).view(np.float16)
    if out_dtype == "bfloat16":
        rne = (u.astype(np.uint64) + np.uint64(0x7fff) + ((u >> np.uint32(16)) & np.uint32(1))) \
            >> np.uint64(16)
        return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), rne).astype(np.uint16)
    raise ValueError(f"mx: unknown output type {out_dtype!r} (float32, float16, bfloat16)")


def _pow2(biased):
    """``2^(biased - 127)`` as float32 from its bits (``biased == 0``: 2^-127)."""
    b = np.asarray(biased, dtype=np.uint32)
    return np.where(b == 0, np.uint32(0x00400000), b << np.uint32(23)).astype(np.uint32) \
        .view(np.float32)


def encode(v, fmt):
    """The codes (uint8) of the float32 values ``v``, ``|v| <= max``: nearest,
    ties to even, the sign bit kept."""
    bits, _, _, mbits, bias = _fmt(fmt)
    v = _f32(v)
    a = v.view(np.uint32) & np.uint32(0x7fffffff)
    drop = np.uint32(23 - mbits)
    # normals: round the f32 mantissa to mbits, a carry running into the exponent
    rounded = (a + ((np.uint32(1) << (drop - np.uint32(1))) - np.uint32(1))
               + ((a >> drop) & np.uint32(1))) >> drop
    normal = rounded.astype(np.int64) - ((127 - bias) << mbits)
    # below the smallest normal 2^(1 - bias): a multiple of the subnormal step
    sub = np.rint(np.abs(v).astype(np.float64) * 2.0 ** (bias - 1 + mbits)).astype(np.int64)
    code = np.where(a >= np.uint32((127 + 1 - bias) << 23), normal, sub)
    sign = (v.view(np.uint32) >> np.uint32(31)).astype(np.int64) << (bits - 1)
    return (code | sign).astype(np.uint8)


def value(codes, fmt):
    """``f32(q)`` of the codes (uint8).  The two e4m3 NaN codes give NaN."""
    bits, _, _, mbits, bias = _fmt(fmt)
    q = np.asarray(codes, dtype=np.uint8).astype(np.int64)
    man, exp = q & ((1 << mbits) - 1), (q >> mbits) & ((1 << (bits - 1 - mbits)) - 1)
    mag = np.where(exp == 0, man * 2.0 ** (1 - bias - mbits),
                   (1.0 + man * 2.0 ** -mbits) * 2.0 ** (exp - bias))
    if fmt == "fp8":
        mag = np.where((q & 0x7f) == 0x7f, np.nan, mag)
    return np.where(q >> (bits - 1) == 1, -mag, mag).astype(np.float32)


def _blocks(c):
    """``c`` padded with +0.0 to whole blocks, as rows of 32."""
    padded = np.zeros(scale_bytes(c.size) * BLOCK, dtype=np.float32)
    padded[:c.size] = c
    return padded.reshape(-1, BLOCK)


def scales(c, fmt):
    """``X_b`` (uint8) of the float32 array ``c``."""
    emax = _fmt(fmt)[1]
    key = _blocks(_f32(c)).view(np.uint32) & np.uint32(0x7fffffff)
    e = (key.max(axis=1, initial=0) >> np.uint32(23)).astype(np.int64)
    return np.where(e == 255, 255, np.clip(e - emax, 0, 254)).astype(np.uint8)


def quantise(c, fmt):
    """``(X uint8 [blocks], q uint8 [n], d float32 [n])`` of the float32 array ``c``."""
    vmax = np.float32(_fmt(fmt)[2])
    c = _f32(c)
    x = scales(c, fmt)
    xe = np.repeat(x, BLOCK)[:c.size].astype(np.uint32)
    bad = xe == 255
    with np.errstate(all="ignore"):
        v = c * _pow2(np.where(bad, 127, 254 - xe.astype(np.int64)))
        v = np.where(bad, np.float32(0.0), np.clip(v, -vmax, vmax)).astype(np.float32)
        q = np.where(bad, 0, encode(v, fmt)).astype(np.uint8)
        d = (value(q, fmt) * _pow2(xe)).astype(np.float32)
    d[bad] = np.uint32(0x7fc00000).view(np.float32)
    return x, q, d


def compress(g, r, fmt, bf16: bool = False):
    """One step: ``(payload, r')`` — the payload as a new uint8 array, the new
    residual as a new float32 array — from the gradient ``g`` (float32,
    float16, or with ``bf16`` its bf16 bits; ``widen``) and the float32
    residual ``r``."""
    g, r = widen(g, bf16), _f32(r)
    if g.size != r.size:
        raise ValueError(f"mx: {g.size} elements, {r.size} residuals")
    if g.size > MAX_ELEMS:
        raise ValueError("mx: more than 2^31 elements")
    n, bits = g.size, bits_of(fmt)
    with np.errstate(all="ignore"):
        c = g + r
        x, q, d = quantise(c, fmt)
        rn = c - d
    rn[np.repeat(x == 255, BLOCK)[:g.size]] = np.uint32(0x7fc00000).view(np.float32)
    payload = np.zeros(payload_bytes(n, fmt), dtype=np.uint8)
    payload[0:4] = np.array([bits], dtype="<u4").view(np.uint8)
    payload[4:12] = np.array([n], dtype="<u8").view(np.uint8)
    at = HEADER_BYTES
    payload[at:at + x.size] = x
    at += _align16(x.size)
    if bits == 4:
        pairs = np.zeros(2 * code_bytes(n, fmt), dtype=np.uint8)
        pairs[:n] = q
        q = pairs[0::2] | (pairs[1::2] << 4)
    payload[at:at + q.size] = q
    return payload, rn.astype(np.float32)


def header(payload):
    """``(bits, n)`` as a payload's header states them (never used for sizes)."""
    p = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
    return int(p[0:4].view("<u4")[0]), int(p[4:12].view("<u8")[0])


def fields(payload, n: int, fmt):
    """``(X uint8 [blocks], q uint8 [n])`` of a payload of ``n`` elements."""
    p = np.ascontiguousarray(payload).reshape(-1).view(np.uint8)
    n = int(n)
    if p.size < payload_bytes(n, fmt):
        raise ValueError(f"mx: a {p.size}-byte payload for {n} {fmt} elements")
    at = HEADER_BYTES + _align16(scale_bytes(n))
    raw = p[at:at + code_bytes(n, fmt)]
    if bits_of(fmt) == 4:
        raw = np.stack([raw & 0xf, raw >> 4], axis=1).reshape(-1)[:n]
    return p[HEADER_BYTES:HEADER_BYTES + scale_bytes(n)], raw


def decode(payload, n: int, fmt):
    """``d``: a new float32 array of ``n`` elements."""
    x, q = fields(payload, n, fmt)
    xe = np.repeat(x, BLOCK)[:int(n)].astype(np.uint32)
    with np.errstate(all="ignore"):
        d = (value(q, fmt) * _pow2(xe)).astype(np.float32)
    d[xe == 255] = np.uint32(0x7fc00000).view(np.float32)
    return d


def fold(payloads, n: int, fmt, divisor: int = 1, out_dtype=None):
    """The N-way decode: the float32 left fold of ``decode(p, n, fmt)`` over
    ``payloads`` in order, divided by ``f32(divisor)`` when ``divisor > 1``,
    then ``narrow(.., out_dtype)``: one conversion of the float32 result."""
    if not 1 <= len(payloads) <= MAX_SRCS:
        raise ValueError(f"mx: {len(payloads)} sources outside 1..{MAX_SRCS}")
    if int(divisor) < 1:
        raise ValueError(f"divisor {divisor} < 1")
    with np.errstate(all="ignore"):
        out = decode(payloads[0], n, fmt)
        for p in payloads[1:]:
            out = out + decode(p, n, fmt)
        if int(divisor) > 1:
            out = out / np.float32(int(divisor))
    return narrow(out.astype(np.float32), out_dtype)


def refold(payloads, n: int, resid, fmt):
    """The server round: ``(payload, r')`` — ``compress(fold(payloads, n, fmt),
    resid, fmt)``, the float32 sum of 1..16 decodes in argument order (no
    divide: a worker's fold of what it pulls applies the ``average`` divisor)
    compressed against the server's float32 residual.  Nothing new is defined:
    a source block with ``X == 255`` makes the sum's block NaN, an overflowed
    sum makes it inf, and ``compress`` pins both — ``X = 255``, codes 0, ``r' =
    0x7fc00000``.  The HIP kernel (``prophet_amd/csrc/bpsr_k_mx_refold.hip``)
    is this line in one launch, the sum never written."""
    return compress(fold(payloads, n, fmt), resid, fmt)


__all__ = ["HEADER_BYTES", "BLOCK", "MAX_SRCS", "MAX_ELEMS", "bits_of", "scale_bytes",
           "code_bytes", "payload_bytes", "widen", "narrow", "encode", "value", "scales",
           "quantise", "compress", "header", "fields", "decode", "fold", "refold"]
