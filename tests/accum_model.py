"""Plain numpy model of BYTEPS_REDUCE_MODE_ACCUM_F32 (fp16 / bf16 folded in
fp32), and order-sensitive inputs for it.  A helper module, not a conftest.

The mode's contract, per element, on bit patterns, for sources s[0..n-1]:

    up(h)      bf16: h << 16.  fp16: the exact fp32 value; a NaN becomes
               sign | 0x7f800000 | (payload << 13) | 0x00400000 (quieted).
    add32(a,b) r = a + b in fp32, round to nearest even, subnormals kept.  If r
               is NaN: a | 0x00400000 if a is NaN, else b | 0x00400000 if b is
               NaN, else 0xffc00000 (inf + -inf).
    down(x)    fp16: NaN -> ((x >> 16) & 0x8000) | 0x7e00 | ((x >> 13) & 0x3ff),
               else RNE to fp16 (overflow gives Inf, subnormals kept).
               bf16: NaN -> (x >> 16) | 0x0040,
               else (x + 0x7fff + ((x >> 16) & 1)) >> 16.
    n == 1     a byte copy (signalling NaNs stay as they are).
    2..32      down(add32(... add32(up(s0), up(s1)) ..., up(s[n-1]))).
    n > 32     the first 32 sources fold and narrow; each further launch folds
               [running result] + the next 31 and narrows again.

Everything works on uint32 / uint16 views; float arithmetic happens only inside
``add32`` (one IEEE fp32 add) and the finite branch of the fp16 ``down`` /
``up`` (numpy's float16 <-> float32 casts, checked against torch's in
tests/test_accum_model.py).
"""
from __future__ import annotations

import numpy as np

from prophet_amd import synth
from prophet_amd.dtypes import DType

MAX_SRCS = 32          # BYTEPS_REDUCE_MAX_SRCS: sources of one launch

_U32 = np.uint32


def f32_nan(x: np.ndarray) -> np.ndarray:
    return (x & _U32(0x7FFFFFFF)) > _U32(0x7F800000)


def up(h: np.ndarray, bf16: bool) -> np.ndarray:
    """uint16 patterns -> fp32 patterns (uint32), exactly."""
    h16 = np.ascontiguousarray(h, dtype=np.uint16)
    h = h16.astype(_U32)
    if bf16:
        return h << _U32(16)
    f = h16.view(np.float16).astype(np.float32).view(_U32)
    nan = (h & _U32(0x7FFF)) > _U32(0x7C00)
    if nan.any():
        q = (((h & _U32(0x8000)) << _U32(16)) | _U32(0x7F800000) |
             ((h & _U32(0x03FF)) << _U32(13)) | _U32(0x00400000))
        f = np.where(nan, q, f)
    return f


def add32(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """One fp32 add on patterns, with the NaN rule."""
    a = np.ascontiguousarray(a, dtype=_U32)
    b = np.ascontiguousarray(b, dtype=_U32)
    with np.errstate(all="ignore"):
        r = a.view(np.float32) + b.view(np.float32)
    u = r.view(_U32)
    bad = np.isnan(r)
    if bad.any():
        fix = np.where(f32_nan(a), a | _U32(0x00400000),
                       np.where(f32_nan(b), b | _U32(0x00400000), _U32(0xFFC00000)))
        u = np.where(bad, fix, u).astype(_U32)
    return u


def down(x: np.ndarray, bf16: bool) -> np.ndarray:
    """fp32 patterns -> uint16 patterns, round to nearest even."""
    x = np.ascontiguousarray(x, dtype=_U32)
    nan = f32_nan(x)
    if bf16:
        r = (x + _U32(0x7FFF) + ((x >> _U32(16)) & _U32(1))) >> _U32(16)
        if nan.any():
            r = np.where(nan, (x >> _U32(16)) | _U32(0x0040), r)
        return r.astype(np.uint16)
    with np.errstate(all="ignore"):
        r = x.view(np.float32).astype(np.float16).view(np.uint16)
    if nan.any():
        q = ((x >> _U32(16)) & _U32(0x8000)) | _U32(0x7E00) | ((x >> _U32(13)) & _U32(0x03FF))
        r = np.where(nan, q.astype(np.uint16), r)
    return r


def fold32(ins, bf16: bool) -> np.ndarray:
    """The strict left fold of one launch in fp32 patterns (not narrowed)."""
    acc = up(ins[0], bf16)
    for s in ins[1:]:
        acc = add32(acc, up(s, bf16))
    return acc


def accum_fold(ins, bf16: bool, narrow=down) -> np.ndarray:
    """The mode's result for sources ``ins`` (uint16 arrays), any n >= 1.
    ``narrow`` replaces ``down`` (the tests' wrong variants use it)."""
    ins = [np.ascontiguousarray(s, dtype=np.uint16) for s in ins]
    if len(ins) == 1:
        return ins[0].copy()
    r = narrow(fold32(ins[:MAX_SRCS], bf16), bf16)
    k = MAX_SRCS
    while k < len(ins):
        m = min(len(ins) - k, MAX_SRCS - 1)
        r = narrow(fold32([r] + ins[k:k + m], bf16), bf16)
        k += m
    return r


def fold_bytes(ins_u8, length: int, bf16: bool, prefill: int = 0x5A) -> np.ndarray:
    """Expected ``length`` output bytes for byte-array sources: the model over
    ``length // 2`` elements, the trailing ``length % 2`` byte from ins[0]."""
    out = np.full(length, prefill, np.uint8)
    ne = length // 2
    if ne:
        srcs = [np.ascontiguousarray(x[:2 * ne]).view(np.uint16) for x in ins_u8]
        out[:2 * ne] = accum_fold(srcs, bf16).view(np.uint8)
    if length % 2:
        out[2 * ne] = ins_u8[0][2 * ne]
    return out


# ------------------------------------------------------------------ inputs ----

def _open_uniform(seed: int, count: int) -> np.ndarray:
    """U(-1, 1), both ends excluded, as float64 (53 bits of a splitmix64 draw)."""
    r = (synth.splitmix64(seed, count) >> np.uint64(11)).astype(np.float64)
    return (r + 0.5) * (2.0 / (1 << 53)) - 1.0


def cancel(dtype, n_elems: int, n_sources: int, seed: int) -> list:
    """Order-sensitive inputs, uint16 patterns, one array per source.

    Per element one source holds +B and another exactly -B (the same bits, the
    sign flipped), at random positions; |B| lies in [2^10, 2^15) for fp16 and in
    [2^20, 2^40) for bf16.  Every other source is uniform in (-1, 1), rounded
    to the format.  So the small addends are absorbed or kept depending on
    whether they meet the accumulator before, between or after the pair, and
    on where the sum is narrowed.

    With two or three sources a pair in every element would leave the
    narrowing nothing to round (the result is an exact zero, or the one small
    value, or that value rounded at the pair's magnitude: all representable),
    so a truncating narrowing could not be told from RNE.  There the pair sits
    in the odd elements only and the even ones hold uniform values alone.
    One source: uniform values."""
    dt = DType(dtype)
    assert dt in (DType.FLOAT16, DType.BFLOAT16)
    bf = dt == DType.BFLOAT16
    base = (int(seed) << 20) ^ (0xB0000 if bf else 0xA0000)
    out = np.empty((n_sources, n_elems), np.uint16)
    for k in range(n_sources):
        x = _open_uniform(base + k, n_elems)
        out[k] = synth.f64_to_bf16_bits(x) if bf else x.astype(np.float16).view(np.uint16)
    if n_sources >= 2 and n_elems:
        n = np.uint64(n_sources)
        P = synth.splitmix64(base + 0xFFFF, n_elems)
        p = P % n
        q = (p + np.uint64(1) + (P >> np.uint64(16)) % np.uint64(n_sources - 1)) % n
        sign = ((P >> np.uint64(32)) & np.uint64(1)) << np.uint64(15)
        if bf:      # 2^20 <= |B| < 2^40, 7 stored mantissa bits
            e = np.uint64(127 + 20) + (P >> np.uint64(36)) % np.uint64(20)
            B = sign | (e << np.uint64(7)) | ((P >> np.uint64(48)) & np.uint64(0x7F))
        else:       # 2^10 <= |B| < 2^15, 10 stored mantissa bits
            e = np.uint64(15 + 10) + (P >> np.uint64(36)) % np.uint64(5)
            B = sign | (e << np.uint64(10)) | ((P >> np.uint64(48)) & np.uint64(0x3FF))
        B = B.astype(np.uint16)
        idx = np.arange(n_elems)
        if n_sources <= 3:
            idx = idx[1::2]
        out[p[idx].astype(np.int64), idx] = B[idx]
        out[q[idx].astype(np.int64), idx] = B[idx] ^ np.uint16(0x8000)
    return [np.ascontiguousarray(out[k]) for k in range(n_sources)]


def inputs(dtype, n_elems: int, n_sources: int, value_class: str, seed: int) -> list:
    """Byte arrays of ``n_sources`` buckets: ``cancel`` or a synth value class."""
    if value_class == "cancel":
        return [x.view(np.uint8) for x in cancel(dtype, n_elems, n_sources, seed)]
    return [np.ascontiguousarray(synth.bucket(dtype, n_elems, k, value_class, seed)).view(np.uint8)
            for k in range(n_sources)]
