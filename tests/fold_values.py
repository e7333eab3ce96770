"""Enumerated operand tables for the fold operators: which values meet each
other, not where they sit.  A helper module, not a conftest; pure numpy, no
randomness.

The position-oriented fold tests draw every source independently, so the
pairs that decide whether an add is right (cancellation to a subnormal or to
zero, an exact rounding tie, max finite plus half an ulp, -0 + -0, a NaN
against every class of partner in both orders, a carry across the words of an
int64) almost never occur there.  Here they are built by bit arithmetic on the
patterns.

pair_table(dt) -> (a, b, kind): two sources as unsigned patterns of the
element width and a small integer per element naming the row's construction
(for fold_run.assert_elements).

  fp16, bf16   every one of the 65,536 patterns `a` (a-major) against the
               PARTNERS_16 partners derived from it (derived_partners, then
               CONSTANTS of both signs, then 1.0), and the specials block.
  f32, f64     the ordered cross product B x B of boundary_set, the derived
               partners of every member of B, and the specials block.
  int8, uint8  all 256 x 256 ordered pairs.
  int32/int64  the cross product of int_boundary_set; int64 also low words
               that carry into the high word and that stop one short of it.

The specials block is specials x specials plus one 1.0 + 1.0 row (an odd
period, so every pair meets both halves of a packed pair and every lane),
repeated SPECIAL_REPS times: it is what brings -0 + -0 and inf - inf, which
the formulas above produce only a handful of times, up to the occurrence
floor of tests/test_fold_values.py.

chain_sources(dt, n) -> (sources, kind): n sources of one left fold.  A block
of hand-written triples (floats only; further sources there are -0, the
identity of IEEE addition) followed by pair_table's a and b; source k >= 2 is
b rolled by (k - 1) * STRIDE elements, STRIDE coprime to both partner counts,
so every element meets a different sequence.  Sources 3 and up keep only one
in THIN_PERIOD of their inf / NaN patterns (_thin), or no long fold would end
in a finite value.

classify(dt, a, b, r) names the value classes of a two-source result r.
"""
from __future__ import annotations

import numpy as np

from prophet_amd.dtypes import DType

STRIDE = 37                 # coprime to PARTNERS_16 (35) and to len(boundary_set) (250)
SPECIAL_REPS = 72           # 325 * 72 elements: a multiple of 8 (the fp16 body)
TRIPLE_REPS = 65

# kinds
K_CONST0 = 16               # kinds 0..15 derived partners, 16..33 constants, 34 one
K_ONE = 34
K_SPECIAL, K_PAD, K_CROSS = 40, 41, 42
K_DERIVED0 = 50             # 50..65: derived partners of boundary_set's members
K_TRIPLE0 = 70              # 70..: hand-written triples
K_INT_CROSS, K_INT_CARRY, K_INT_SHORT = 90, 91, 92

_U64 = np.uint64


class Fmt:
    """Bit layout of a binary floating-point format of `bits` bits with `m`
    stored mantissa bits."""

    def __init__(self, bits: int, m: int):
        self.bits, self.m = bits, m
        self.U = np.dtype(f"u{bits // 8}")
        self.mask = (1 << bits) - 1
        self.sign = 1 << (bits - 1)
        self.emax = (1 << (bits - 1 - m)) - 1           # the inf / NaN exponent field
        self.bias = self.emax >> 1
        self.mant = (1 << m) - 1
        self.inf = self.emax << m
        self.quiet = 1 << (m - 1)
        self.one = self.bias << m
        self.min_sub, self.max_sub, self.min_norm = 1, self.mant, 1 << m
        self.max_fin = self.inf - 1
        self.qnan = self.inf | self.quiet
        # a signalling NaN with a payload, and a quiet NaN with another payload
        self.snan = self.inf | (0x5555555555555555 & (self.quiet - 1)) | 1
        self.nan2 = self.inf | self.quiet | (0xAAAAAAAAAAAAAAAA & (self.quiet - 1))


FMT = {DType.FLOAT16: Fmt(16, 10), DType.BFLOAT16: Fmt(16, 7),
       DType.FLOAT32: Fmt(32, 23), DType.FLOAT64: Fmt(64, 52)}
FLOATS_16 = (DType.FLOAT16, DType.BFLOAT16)
INT_BITS = {DType.INT8: 8, DType.UINT8: 8, DType.INT32: 32, DType.INT64: 64}


def constants(f: Fmt) -> list:
    """zero, min and max subnormal, min normal, max finite, inf, a quiet NaN,
    a signalling NaN with a payload, a NaN with a different payload; then the
    same with the sign set.  The last one is a NaN."""
    pos = [0, f.min_sub, f.max_sub, f.min_norm, f.max_fin, f.inf, f.qnan, f.snan, f.nan2]
    return pos + [x | f.sign for x in pos]


def half_ulp(f: Fmt, a: np.ndarray) -> np.ndarray:
    """The pattern of half a unit in the last place of `a` (uint64 patterns),
    by `a`'s exponent field e alone: 2^(e - bias - m - 1), a normal number
    from e = m + 2 on, a subnormal one down to e = 2, and zero (not
    representable) below.  inf and NaN fall through the same formula."""
    e = ((a >> _U64(f.m)) & _U64(f.emax)).astype(np.int64)
    normal = np.clip(e - f.m - 1, 0, None) << f.m
    sub = np.int64(1) << np.clip(e - 2, 0, f.m)
    return np.where(e >= f.m + 2, normal, np.where(e >= 2, sub, 0)).astype(_U64)


def derived_partners(f: Fmt, a: np.ndarray) -> np.ndarray:
    """16 partners per element of `a`, shape (len(a), 16), uint64 patterns:
    -a and a, each moved by -2 .. +2 pattern steps (cancellations to
    subnormals and zero; doublings that overflow at the top), then half an ulp
    of a in both signs, each also one pattern step above and below (the exact
    tie and its two neighbours)."""
    a = a.astype(_U64)
    mask = _U64(f.mask)
    step = lambda x, d: (x + _U64(d & f.mask)) & mask       # noqa: E731
    cols = [step(a ^ _U64(f.sign), d) for d in (-2, -1, 0, 1, 2)]
    cols += [step(a, d) for d in (-2, -1, 0, 1, 2)]
    hu = half_ulp(f, a)
    for s in (0, f.sign):
        cols += [step(hu | _U64(s), d) for d in (0, 1, -1)]
    return np.stack(cols, axis=1)


N_DERIVED = 16
PARTNERS_16 = N_DERIVED + 18 + 1        # odd: a partner meets both halves of a packed pair


def specials_block(f: Fmt):
    """constants x constants (ordered) and one 1.0 + 1.0 row, SPECIAL_REPS
    times."""
    c = np.array(constants(f), dtype=_U64)
    a = np.concatenate([np.repeat(c, len(c)), [_U64(f.one)]])
    b = np.concatenate([np.tile(c, len(c)), [_U64(f.one)]])
    kind = np.full(len(a), K_SPECIAL, np.int16)
    kind[-1] = K_PAD
    return np.tile(a, SPECIAL_REPS), np.tile(b, SPECIAL_REPS), np.tile(kind, SPECIAL_REPS)


def boundary_set(f: Fmt) -> np.ndarray:
    """B of the f32 / f64 tables: 15 exponent fields x 8 mantissas, inf, a
    quiet NaN, two signalling NaNs and a quiet NaN with a payload; everything
    in both signs (250 patterns)."""
    p, bias, emax, half = f.m, f.bias, f.emax, f.quiet
    exps = [0, 1, 2, p, p + 1, p + 2, bias - p - 1, bias - 1, bias, bias + 1, bias + p,
            bias + p + 1, emax - p - 2, emax - 2, emax - 1]
    mants = [0, 1, 2, half - 1, half, half + 1, f.mant - 1, f.mant]
    pos = [(e << f.m) | m for e in exps for m in mants]
    pos += [f.inf, f.qnan, f.inf | 1, f.snan, f.nan2]
    assert len(set(pos)) == len(pos)
    return np.array(pos + [x | f.sign for x in pos], dtype=_U64)


def int_boundary_set(bits: int) -> np.ndarray:
    """0, +-1, min, max, all ones, the word and half-word boundaries and two
    alternating patterns, each with its neighbours at -2 .. +2."""
    mask = (1 << bits) - 1
    h = bits // 2
    base = [0, 1 << (bits - 1), (1 << (bits - 1)) - 1, mask, (1 << h) - 1, 1 << h,
            mask ^ ((1 << h) - 1), (1 << (h - 1)) - 1, 1 << (h - 1),
            0x5555555555555555 & mask, 0xAAAAAAAAAAAAAAAA & mask]
    vals = sorted({(x + d) & mask for x in base for d in (-2, -1, 0, 1, 2)})
    return np.array(vals, dtype=_U64)


def int64_carry_pairs():
    """Low words whose sum is exactly 2^32 (a carry into the high word) and
    2^32 - 1 (one short of it), under every pair of a few high words, among
    them 0x00000000ffffffff + 1, 0x7fffffffffffffff + 1 and
    0xffffffff00000000 + 0x0000000100000000 (no carry out of the low word, a
    wrap of the high one)."""
    lows = [1, 2, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF]
    highs = [0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF]
    a, b, kind = [], [], []
    for la in lows:
        for short in (0, 1):
            lb = (1 << 32) - la - short
            for ha in highs:
                for hb in highs:
                    a.append((ha << 32) | la)
                    b.append((hb << 32) | lb)
                    kind.append(K_INT_SHORT if short else K_INT_CARRY)
    return np.array(a, dtype=_U64), np.array(b, dtype=_U64), np.array(kind, np.int16)


def _cross(v: np.ndarray):
    return np.repeat(v, len(v)), np.tile(v, len(v))


_PAIRS: dict = {}


def pair_table(dt):
    """(a, b, kind) of `dt`; shared, never modified."""
    dt = DType(dt)
    if dt in _PAIRS:
        return _PAIRS[dt]
    if dt in INT_BITS:
        bits = INT_BITS[dt]
        if bits == 8:
            a, b = _cross(np.arange(256, dtype=_U64))
            kind = np.full(len(a), K_INT_CROSS, np.int16)
        else:
            a, b = _cross(int_boundary_set(bits))
            kind = np.full(len(a), K_INT_CROSS, np.int16)
            if bits == 64:
                ca, cb, ck = int64_carry_pairs()
                a, b, kind = (np.concatenate(x) for x in ((a, ca), (b, cb), (kind, ck)))
        U = np.dtype(f"u{bits // 8}")
    else:
        f = FMT[dt]
        U = f.U
        if f.bits == 16:
            pat = np.arange(1 << 16, dtype=_U64)
            c = np.array(constants(f) + [f.one], dtype=_U64)
            part = np.concatenate([derived_partners(f, pat),
                                   np.broadcast_to(c, (len(pat), len(c)))], axis=1)
            assert part.shape[1] == PARTNERS_16
            blocks = [(np.repeat(pat, PARTNERS_16), part.ravel(),
                       np.tile(np.arange(PARTNERS_16, dtype=np.int16), len(pat)))]
        else:
            B = boundary_set(f)
            ca, cb = _cross(B)
            d = derived_partners(f, B)
            blocks = [(ca, cb, np.full(len(ca), K_CROSS, np.int16)),
                      (np.repeat(B, N_DERIVED), d.ravel(),
                       np.tile(np.arange(K_DERIVED0, K_DERIVED0 + N_DERIVED, dtype=np.int16),
                               len(B)))]
        blocks.append(specials_block(f))
        a, b, kind = (np.concatenate([blk[i] for blk in blocks]) for i in range(3))
    out = (np.ascontiguousarray(a.astype(U)), np.ascontiguousarray(b.astype(U)), kind)
    for x in out:
        x.setflags(write=False)
    _PAIRS[dt] = out
    return out


def fp16_tail_cut() -> int:
    """Elements of the fp16 table at the length with n % 8 == 5: its last five
    rows (a NaN constant against NaN constants, in the specials block) then
    lie in the reference's scalar tail, where every NaN becomes 0x7fff."""
    n = len(pair_table(DType.FLOAT16)[0])
    assert n % 8 == 0
    return n - 3


def triples(dt) -> np.ndarray:
    """The hand-written triples of a float dtype, shape (9, 3), patterns."""
    f = FMT[DType(dt)]
    S = f.sign
    hu_one = (f.bias - f.m - 1) << f.m                  # half an ulp of 1.0
    # the header's own fp16 example, 65504, 1e-4, -65504; elsewhere max finite
    # and a small normal number in its place
    small = 0x068E if DType(dt) == DType.FLOAT16 else ((f.bias - 13) << f.m) | (f.quiet + 3)
    x = f.one | (f.quiet + 1)
    rows = [
        (f.max_fin, f.min_sub, f.max_fin | S),          # max, tiny, -max
        (x, x | S, S),                                  # x, -x, -0
        (f.inf, f.nan2, f.inf | S),                     # inf, NaN, -inf
        (f.max_fin, small, f.max_fin | S),              # 65504, 1e-4, -65504
        (f.max_fin, f.max_fin, f.max_fin | S),          # overflows first; reversed it does not
        (S, S, S),                                      # -0 + -0 + -0 = -0
        (f.snan, f.nan2 | S, f.inf),                    # two NaNs: the first wins, quieted
        (f.inf, f.inf | S, f.snan),                     # the default NaN, then it wins
        (f.one, hu_one, hu_one),                        # two ties to even; reversed, one ulp more
    ]
    return np.array(rows, dtype=_U64)


_CHAINS: dict = {}
CHAIN_MAX = 33              # one source more than a single launch folds
THIN_PERIOD = 11


def _thin(dt, x: np.ndarray, k: int) -> np.ndarray:
    """Source k >= 3 of a float chain keeps its inf and NaN patterns only in
    the elements i with i % THIN_PERIOD == k % THIN_PERIOD and holds -0 (the
    identity) in their place elsewhere.  Every partner list has 8 such
    patterns, so a fold of 17 rolled sources or more would otherwise end in a
    NaN in every element and its finite arithmetic would go unseen; sources 0
    to 2 stay as dense as they are."""
    if dt not in FMT or k < 3:
        return x
    f = FMT[dt]
    U = f.U.type
    nonfinite = (x & U(f.sign - 1)) >= U(f.inf)
    keep = (np.arange(len(x)) % THIN_PERIOD) == (k % THIN_PERIOD)
    return np.where(nonfinite & ~keep, U(f.sign), x)


def chain_sources(dt, n: int):
    """(sources, kind) of an n-way fold, n >= 3; shared, never modified."""
    dt = DType(dt)
    assert 3 <= n <= CHAIN_MAX
    if dt not in _CHAINS:       # the sources of a shorter fold are the first of a longer one's
        _CHAINS[dt] = _chain_sources(dt, CHAIN_MAX)
    srcs, kind = _CHAINS[dt]
    return srcs[:n], kind


def _chain_sources(dt, n: int):
    a, b, kind = pair_table(dt)
    if dt in FMT:
        f = FMT[dt]
        t = np.tile(triples(dt), (TRIPLE_REPS, 1)).astype(f.U)
        tk = np.tile(np.arange(K_TRIPLE0, K_TRIPLE0 + 9, dtype=np.int16), TRIPLE_REPS)
        ident = np.full(len(t), f.sign, f.U)
        head = [t[:, 0], t[:, 1], t[:, 2]] + [ident] * (n - 3)
    else:
        tk = np.zeros(0, np.int16)
        head = [np.zeros(0, a.dtype)] * n
    body = [a, b] + [_thin(dt, np.roll(b, (k - 1) * STRIDE), k) for k in range(2, n)]
    srcs = [np.ascontiguousarray(np.concatenate([h, x])) for h, x in zip(head, body)]
    out = (srcs, np.concatenate([tk, kind]))
    for x in srcs:
        x.setflags(write=False)
    return out


def as_bytes(x: np.ndarray) -> np.ndarray:
    return x.view(np.uint8)


# ---------------------------------------------------------------- classes ----

def to_f64(dt, u: np.ndarray) -> np.ndarray:
    """The values of 16-bit patterns, exactly."""
    if DType(dt) == DType.FLOAT16:
        return u.view(np.float16).astype(np.float64)
    with np.errstate(invalid="ignore"):         # signalling NaNs
        return (u.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def classify(dt, a: np.ndarray, b: np.ndarray, r: np.ndarray) -> dict:
    """Boolean masks over the elements of a two-source fold r = a + b (a is
    dst, the first arrival), by value class."""
    f = FMT[DType(dt)]
    U = f.U.type
    mag = lambda x: x & U(f.sign - 1)                   # noqa: E731
    nan = lambda x: mag(x) > U(f.inf)                   # noqa: E731
    snan = lambda x: nan(x) & ((x & U(f.quiet)) == 0)   # noqa: E731
    inf = lambda x: mag(x) == U(f.inf)                  # noqa: E731
    finite = lambda x: mag(x) < U(f.inf)                # noqa: E731
    nonzero = lambda x: finite(x) & (mag(x) != 0)       # noqa: E731
    both_fin = finite(a) & finite(b)
    out = {
        "subnormal_result": nonzero(a) & nonzero(b) & (mag(r) != 0) & (mag(r) < U(f.min_norm)),
        "cancel_to_plus_zero": nonzero(a) & nonzero(b) & (r == 0),
        "minus_zero_result": r == U(f.sign),
        "overflow_to_plus_inf": both_fin & (r == U(f.inf)),
        "overflow_to_minus_inf": both_fin & (r == U(f.inf | f.sign)),
        "nan_in_dst_only": nan(a) & ~nan(b),
        "nan_in_src_only": ~nan(a) & nan(b),
        "nan_in_both": nan(a) & nan(b),
        "snan_in_dst": snan(a),
        "snan_in_src": snan(b),
        "inf_minus_inf": inf(a) & inf(b) & (((a ^ b) & U(f.sign)) != 0),
    }
    if f.bits == 16:
        fa, fb, fr = (to_f64(dt, x) for x in (a, b, r))
        with np.errstate(all="ignore"):
            # exact in f64 wherever the operands are close enough for a tie
            s = np.abs(fa + fb)
            inexact = both_fin & finite(r) & (s != np.abs(fr))
            up = s < np.abs(fr)                         # rounded away from zero
            # r's neighbour on the other side of the exact sum
            nb = np.where(up, mag(r) - U(1), mag(r) + U(1)).astype(f.U)
            tie = inexact & finite(nb) & (np.abs(s - np.abs(fr)) == np.abs(to_f64(dt, nb) - s))
        out["tie_rounds_up"] = tie & up
        out["tie_rounds_down"] = tie & ~up
    return out
