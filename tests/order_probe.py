"""Inputs that make a fold's order visible through the NaN rule, and the key
shapes the order tests share.  A helper module (pure numpy), not a conftest.

The reference's payload rule, restated by oracle/bpsr_oracle.c: an add gives
quiet(dst) if dst is NaN, else quiet(src) if src is NaN, else the default NaN
(inf + -inf).  It holds for fp32 / fp64, the fp16 body and bf16; in the fp16
scalar tail (elements from floor(n / 8) * 8 on) every NaN becomes 0x7fff.  So a
left fold's NaN result names the first NaN that arrived, and probe elements
built on that rule pin the arrival order:

  all            every worker holds a NaN whose low mantissa bits are
                 worker + 1 (even workers quiet, odd ones signalling, every
                 third one negative): the result names the first arrival.
  pair(a, b)     only a and b hold their NaN: the result names which of the
                 two came first.  All pairs together pin the whole order.
  clash(a, b, c) a holds +inf, b -inf, c its NaN (b, c the next two workers):
                 the default NaN exactly when a and b both precede c,
                 else quiet(c).  Three workers at least.
  negzero        every worker holds -0: the result is -0 (an accumulator
                 started at +0 instead of the first arrival gives +0).
  minsub         every worker holds the smallest subnormal: N times it (a
                 flush to zero shows).
  maxfin         +-(largest finite), alternating by worker: finite or +-inf
                 depending on the order, with no NaN — the fast path's order.

The background is synth's ``normal`` class.  A region (a range of elements)
gets the probe list over and over at every third element — a stride that is odd
with respect to the 16-byte vector (8, 4 or 2 elements), so NaN lanes and
finite lanes share vectors and a replayed vector's finite lanes must still
match.  The list is in priority order (all, negzero, maxfin, minsub, the
clashes, the pairs by growing distance).  A region too short for one whole
cycle goes on with the list in a second pass, one element behind the first
(every third element stays background, so every vector of 4 or 8 elements
still holds a finite lane), and holds the list's head if that is too short as
well; a region of fewer than DENSE_BELOW elements (a head, a ragged tail, a
tiny key) gets the list at every element.
"""
from __future__ import annotations

import numpy as np

from prophet_amd import synth
from prophet_amd.dtypes import DType, elem_size

STRIDE = 3
DENSE_BELOW = 24
TILE_BYTES = 256 * 16           # one workgroup's tile at VPT 1 (bpsr_internal.h kBlock)

# bits type, exponent mask, quiet bit, sign bit, largest finite, smallest subnormal
_FMT = {
    DType.FLOAT16: (np.uint16, 0x7C00, 0x0200, 0x8000, 0x7BFF, 1),
    DType.BFLOAT16: (np.uint16, 0x7F80, 0x0040, 0x8000, 0x7F7F, 1),
    DType.FLOAT32: (np.uint32, 0x7F800000, 0x00400000, 0x80000000, 0x7F7FFFFF, 1),
    DType.FLOAT64: (np.uint64, 0x7FF0000000000000, 0x0008000000000000, 0x8000000000000000,
                    0x7FEFFFFFFFFFFFFF, 1),
}


def bits_type(dt):
    return _FMT[DType(dt)][0]


def worker_nan(dt, w: int) -> int:
    """Worker w's NaN: payload w + 1, quiet for even w, negative for w % 3 == 2."""
    _, emask, quiet, sign, _, _ = _FMT[DType(dt)]
    assert 0 < w + 1 < quiet
    return emask | (quiet if w % 2 == 0 else 0) | (sign if w % 3 == 2 else 0) | (w + 1)


def is_nan(dt, raw: np.ndarray) -> np.ndarray:
    """Per element: do these bytes (any uint8 array of whole elements) hold a NaN?"""
    U, emask, _, sign, _, _ = _FMT[DType(dt)]
    u = np.ascontiguousarray(raw).view(U)
    return (u & U(~sign & int(np.iinfo(U).max))) > U(emask)


def kinds(n_workers: int) -> list:
    """The probe list of n_workers >= 2, in priority order."""
    n = n_workers
    assert n >= 2
    out = [("all",), ("negzero",), ("maxfin",), ("minsub",)]
    if n >= 3:
        out += [("clash", a, (a + 1) % n, (a + 2) % n) for a in range(n)]
    for d in range(1, n):
        out += [("pair", a, a + d) for a in range(n - d)]
    return out


def inputs(dt, n_elems: int, n_workers: int, seed: int, regions):
    """(per-worker byte arrays, per-element probe kind or -1).  The kind is an
    index into kinds(n_workers); a later region overrides an earlier one."""
    dt = DType(dt)
    U, emask, _, sign, maxfin, minsub = _FMT[dt]
    N = n_workers
    K = kinds(N)
    kind = np.full(n_elems, -1, np.int32)
    for lo, hi in regions:
        assert 0 <= lo <= hi <= n_elems, (lo, hi, n_elems)
        kind[lo:hi] = -1
        idx = np.arange(lo, hi, STRIDE if hi - lo >= DENSE_BELOW else 1)
        if hi - lo >= DENSE_BELOW and len(idx) < len(K):    # the second pass
            idx = np.concatenate([idx, np.arange(lo + 1, hi, STRIDE)])[:len(K)]
        kind[idx] = np.arange(len(idx)) % len(K)
    data = np.stack([np.ascontiguousarray(synth.bucket(dt, n_elems, w, "normal", seed)).view(U)
                     for w in range(N)]) if n_elems else np.zeros((N, 0), U)
    nan = [U(worker_nan(dt, w)) for w in range(N)]
    for k in np.unique(kind[kind >= 0]):
        e = np.flatnonzero(kind == k)
        what = K[k]
        if what[0] == "all":
            for w in range(N):
                data[w, e] = nan[w]
        elif what[0] == "pair":
            for w in what[1:]:
                data[w, e] = nan[w]
        elif what[0] == "clash":
            a, b, c = what[1:]
            data[a, e] = U(emask)
            data[b, e] = U(emask | sign)
            data[c, e] = nan[c]
        elif what[0] == "negzero":
            data[:, e] = U(sign)
        elif what[0] == "minsub":
            data[:, e] = U(minsub)
        else:
            for w in range(N):
                data[w, e] = U(maxfin | (sign if w % 2 else 0))
    return [np.ascontiguousarray(data[w]).view(np.uint8) for w in range(N)], kind


def orders(n_workers: int) -> list:
    """Three fixed arrival orders: reversed; a derangement (a rotation by about
    a third); and odds then evens, in which no two workers adjacent in 0..N-1
    stay adjacent (N >= 4; with 2 or 3 workers no such order exists: N = 2
    gives the identity there, so that both of its orders come, and N = 3 a
    swap of the first two)."""
    n = n_workers
    rev = list(range(n))[::-1]
    rot = [(i + max(1, n // 3)) % n for i in range(n)]
    if n >= 4:
        mix = list(range(1, n, 2)) + list(range(0, n, 2))
    else:
        mix = [0, 1] if n == 2 else [1, 0, 2]
    return [rev, rot, mix]


def swapped(order, i: int) -> list:
    """`order` with arrivals i and i + 1 exchanged."""
    o = list(order)
    o[i], o[i + 1] = o[i + 1], o[i]
    return o


def second_word_reset(order) -> list:
    """`order` with positions 8.. replaced by their identity values: what a
    consumer that dropped a wide block's second release word would fold."""
    return list(order[:8]) + list(range(8, len(order)))


def fold(port, dt, ins, order) -> np.ndarray:
    """The oracle's left fold of `ins` taken in `order`, as bytes."""
    want = np.zeros(len(ins[0]), np.uint8)
    assert port.sum_n(want, [ins[w] for w in order], len(want), dt) == 0
    return want


def changed(dt, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Per element: do the byte arrays a and b differ?"""
    U = bits_type(dt)
    return np.ascontiguousarray(a).view(U) != np.ascontiguousarray(b).view(U)


# ------------------------------------------------------------------- cases ----
# (workers, dtype) of the server tests (tests/test_server_order_gpu.py) and the
# source counts of the direct calls (tests/test_parity_probe_gpu.py); the CPU
# test of the probes (tests/test_order_probe.py) walks the same lists.
_F16, _BF16, _F32, _F64 = DType.FLOAT16, DType.BFLOAT16, DType.FLOAT32, DType.FLOAT64
DEVICE_NARROW = [(2, _F16), (3, _F32), (8, _F32), (8, _F16), (8, _BF16), (8, _F64)]
DEVICE_WIDE = [(9, _F16), (16, _F32), (16, _BF16)]
LAUNCH = [(8, _F16), (12, _F32)]
COPIED = [(8, _F16)]
ROUNDS = 3
DIRECT_DTYPES = [_F32, _F16, _BF16, _F64]
DIRECT_N = [2, 3, 8, 9, 16, 32, 40]
DIRECT_N_IN_PLACE = [2, 8, 16, 40]
# co-aligned byte offsets: 2, 6 and 14, none of them element-aligned for fp32,
# which takes 4 and 12 instead
DIRECT_OFFSETS = {_F16: [2, 6, 14], _F32: [4, 12]}


def case_id(case) -> str:
    return f"{case[0]}-{DType(case[1]).name}"


def round_order(n_workers: int, rnd: int, key_index: int) -> list:
    """The arrival order of key number `key_index` in round `rnd` (1-based):
    the rounds walk through orders(), rotated per key so that the keys of one
    round differ."""
    return orders(n_workers)[(rnd - 1 + key_index) % 3]


_CACHE = {}


def cached(tag, make):
    """A result computed once per process and shared (never modified)."""
    if tag not in _CACHE:
        _CACHE[tag] = make()
    return _CACHE[tag]


def server_inputs(dt, n_workers: int, rnd: int, key_index: int):
    """inputs() of one server key and round, over all its regions; shared."""
    n, reg = server_keys(dt)[key_index]
    return cached(("srv", int(dt), n_workers, rnd, key_index),
                  lambda: inputs(dt, n, n_workers, 7000 + 100 * rnd + key_index,
                                 list(reg.values())))


# ------------------------------------------------------------------ shapes ----

def tile_elems(dt) -> int:
    return TILE_BYTES // elem_size(dt)


def vec_elems(dt) -> int:
    return 16 // elem_size(dt)


def ragged_tail(dt) -> int:
    """5 / 3 / 1 elements (16-bit / 32-bit / 64-bit): not a whole vector, and
    for fp16 a scalar tail of 5."""
    return {2: 5, 4: 3, 8: 1}[elem_size(dt)]


def ragged_key(dt, head: int = 0):
    """(elements, named regions) of 3 full tiles + 100 vectors + ragged_tail.
    `head` elements precede the first whole vector (operands co-aligned at a
    byte offset inside their 16-byte line); they are a region of their own.
    fp16 with a head has 3 ragged elements, not 5: with n % 8 = 3 the heads of
    7 and 5 elements leave 4 and 6 elements behind the last whole vector, the
    first of them body elements (NaN payloads kept) and the last 3 the scalar
    tail; the head of 1 leaves 2, and the scalar tail's first element inside
    the last vector.  (No n % 8 gives all three heads all three zones.)
    fp16's scalar tail is a region of its own, so that it begins with `all`."""
    t, v = tile_elems(dt), vec_elems(dt)
    n = 3 * t + 100 * v + (3 if head and DType(dt) == DType.FLOAT16 else ragged_tail(dt))
    vec_end = head + (n - head) // v * v
    st = f16_scalar_tail(dt, n).start
    reg = {"first_tile": (0, t), "last_full_tile": (2 * t, 3 * t), "partial_tile": (3 * t, vec_end),
           "tail": (vec_end, max(vec_end, st))}
    if st < n:
        reg["scalar_tail"] = (st, n)
    if head:
        reg["head"] = (0, head)
    return n, reg


def server_keys(dt) -> list:
    """The server tests' keys: (elements, named regions) of 1 element, 7
    elements, one tile + 1 and ragged_key."""
    t = tile_elems(dt)
    return [(1, {"all": (0, 1)}), (7, {"all": (0, 7)}),
            (t + 1, {"tile": (0, t), "last": (t, t + 1)}), ragged_key(dt)]


BIG_BYTES = (16 << 20) + 12


def big_key():
    """(elements, named regions) of one fp32 key of 16 MiB + 12 bytes: 2^20
    vectors, which a table of just over 2,048 tiles of 8 KiB folds at VPT 2 —
    2,048 full tiles of 512 vectors (2,048 elements) and 3 tail elements.
    Probes in the first tile, the last full tile and the tail only."""
    n = BIG_BYTES // 4
    t = 512 * 4
    full = n // 4 * 4
    assert full % t == 0
    return n, {"first_tile": (0, t), "last_full_tile": (full - t, full), "tail": (full, n)}


def big_inputs(n_workers: int = 8):
    n, reg = big_key()
    return cached(("big", n_workers),
                  lambda: inputs(DType.FLOAT32, n, n_workers, 7900, list(reg.values())))


def direct_inputs(dt, n_sources: int, head: int = 0):
    """(sources, kinds, elements, regions) of a direct call on ragged_key."""
    n, reg = ragged_key(dt, head)
    ins, kind = cached(("direct", int(dt), n_sources, head),
                       lambda: inputs(dt, n, n_sources, 8000 + n_sources + head,
                                      list(reg.values())))
    return ins, kind, n, reg


ELEMENT_PATH_ELEMS = 1007       # of test_parity_gpu.test_not_coaligned_and_unaligned


def element_path_inputs(dt, n_sources: int = 4):
    """(sources, kinds, elements, regions) of a bucket that is element work
    only: 1,000 elements of probes at every third one, and the last 7 dense
    (for fp16 the scalar tail)."""
    n = ELEMENT_PATH_ELEMS
    reg = {"body": (0, n // 8 * 8), "tail": (n // 8 * 8, n)}
    ins, kind = cached(("elem", int(dt), n_sources),
                       lambda: inputs(dt, n, n_sources, 8900, list(reg.values())))
    return ins, kind, n, reg


def f16_scalar_tail(dt, n_elems: int) -> range:
    """The reference's scalar tail: fp16 only, from floor(n / 8) * 8 on."""
    if DType(dt) != DType.FLOAT16:
        return range(n_elems, n_elems)
    return range(n_elems // 8 * 8, n_elems)


def vector_tail(dt, n_elems: int, head: int = 0) -> range:
    """The elements behind the last whole vector that are not in the fp16
    scalar tail (fp32 / fp64 / bf16 at head 0: the last n % 4 / 2 / 8)."""
    v = vec_elems(dt)
    lo = head + (n_elems - head) // v * v
    return range(lo, max(lo, f16_scalar_tail(dt, n_elems).start))
