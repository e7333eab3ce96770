"""The numpy model of the fp32-accumulate mode (tests/accum_model.py) is
checked here, on the CPU, before tests/test_accum_gpu.py lets it judge the
kernels: its conversions against torch's CPU casts and the formats' rounding
boundaries, its sums against exactly representable ones, its special values
against rows derived by hand from the contract, and its inputs (``cancel``)
for the power to tell the contract's fold from a wrong one.
"""
import numpy as np
import pytest

import accum_model as am
from prophet_amd.dtypes import DType

torch = pytest.importorskip("torch")

FORMATS = pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
SMALL = 3 * 2048 + 805          # the small shape of tests/test_accum_gpu.py


def u16(*v):
    return np.array(v, np.uint16)


def u32(*v):
    return np.array(v, np.uint32)


def torch_down(x: np.ndarray, bf16: bool) -> np.ndarray:
    t = torch.from_numpy(x.view(np.float32).copy())
    t = t.to(torch.bfloat16 if bf16 else torch.float16)
    return t.view(torch.int16).numpy().view(np.uint16)


# ----------------------------------------------------------- conversions ----

@FORMATS
def test_down_up_round_trips_every_pattern(bf16):
    """down(up(h)) == h for all 65,536 patterns; a NaN comes back quieted
    (fp16: | 0x0200, bf16: | 0x0040), sign and payload kept."""
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    nan = (h & 0x7FFF) > (0x7F80 if bf16 else 0x7C00)
    want = np.where(nan, h | np.uint16(0x0040 if bf16 else 0x0200), h)
    got = am.down(am.up(h, bf16), bf16)
    assert np.array_equal(got, want)
    if bf16:    # a shift, nothing else: signalling NaNs are quieted by add32 / down
        assert np.array_equal(am.up(h, True), h.astype(np.uint32) << np.uint32(16))
    else:       # up() of an fp16 NaN carries the quiet bit in fp32 already
        assert bool(((am.up(h, False)[nan] & 0x00400000) != 0).all())
    assert nan.sum() == (2 * 127 if bf16 else 2 * 1023)


@FORMATS
def test_down_equals_torch_cast_on_random_finite_patterns(bf16):
    rng = np.random.default_rng(20 + bf16)
    x = rng.integers(0, 1 << 32, size=1 << 20, dtype=np.uint64).astype(np.uint32)
    x = x[(x & 0x7F800000) != 0x7F800000]                      # finite
    assert len(x) > 1_000_000 and ((x & 0x7F800000) == 0).any()  # fp32 subnormals included
    assert np.array_equal(am.down(x, bf16), torch_down(x, bf16))
    # dense around the format's own range: every exponent the format has,
    # random mantissas (the uniform draw above is thin near fp16's limits)
    lo, hi = (127 - 30, 127 + 17) if not bf16 else (0, 255)
    e = rng.integers(lo, hi, size=1 << 20, dtype=np.uint64)
    m = rng.integers(0, 1 << 23, size=1 << 20, dtype=np.uint64)
    s = rng.integers(0, 2, size=1 << 20, dtype=np.uint64)
    y = ((s << 31) | (e << 23) | m).astype(np.uint32)
    assert np.array_equal(am.down(y, bf16), torch_down(y, bf16))


def test_down_fp16_rounding_boundaries():
    rows = [
        (0x3F801000, 0x3C00),   # 1 + 2^-11: tie, to even (down)
        (0x3F801001, 0x3C01),   # just above the tie
        (0x3F803000, 0x3C02),   # 1 + 3 * 2^-11: tie, to even (up)
        (0x477FE000, 0x7BFF),   # 65504, the largest finite value
        (0x477FEFFF, 0x7BFF),   # just below 65520
        (0x477FF000, 0x7C00),   # 65520: tie between 65504 and 2^16 -> Inf
        (0xC77FF000, 0xFC00),
        (0x7F7FFFFF, 0x7C00),   # fp32 max
        (0x33800000, 0x0001),   # 2^-24, the smallest subnormal
        (0x33000000, 0x0000),   # half of it: tie, to even (zero)
        (0xB3000000, 0x8000),   # ... keeping the sign
        (0x33000001, 0x0001),   # just above half
        (0x33C00000, 0x0002),   # 1.5 * 2^-24: tie, to even (up)
        (0x387FC000, 0x03FF),   # the largest subnormal
        (0x387FE000, 0x0400),   # halfway to the smallest normal: tie, to even
        (0x00000001, 0x0000), (0x80000001, 0x8000),
        (0x7F800000, 0x7C00), (0xFF800000, 0xFC00),
    ]
    x = u32(*[r[0] for r in rows])
    want = u16(*[r[1] for r in rows])
    assert np.array_equal(am.down(x, False), want)
    assert np.array_equal(torch_down(x, False), want)


def test_down_bf16_rounding_boundaries():
    rows = [
        (0x3F808000, 0x3F80),   # tie, to even (down)
        (0x3F808001, 0x3F81),
        (0x3F818000, 0x3F82),   # tie, to even (up)
        (0x7F7F0000, 0x7F7F),   # the largest finite value
        (0x7F7F7FFF, 0x7F7F),
        (0x7F7F8000, 0x7F80),   # tie above the largest finite value -> Inf
        (0xFF7F8000, 0xFF80),
        (0x7F7FFFFF, 0x7F80),   # fp32 max
        (0x00010000, 0x0001),   # the smallest subnormal
        (0x00008000, 0x0000),   # half of it: tie, to even (zero)
        (0x80008000, 0x8000),
        (0x00008001, 0x0001),
        (0x00018000, 0x0002),   # 1.5 of it: tie, to even (up)
        (0x007F8000, 0x0080),   # halfway to the smallest normal
        (0x00000001, 0x0000), (0x80000001, 0x8000),
        (0x7F800000, 0x7F80), (0xFF800000, 0xFF80),
    ]
    x = u32(*[r[0] for r in rows])
    want = u16(*[r[1] for r in rows])
    assert np.array_equal(am.down(x, True), want)
    assert np.array_equal(torch_down(x, True), want)


# ------------------------------------------------------------ exact sums ----

@FORMATS
@pytest.mark.parametrize("n", [2, 3, 8, 32, 40])
def test_fold_equals_rounded_exact_sum_where_fp32_is_exact(bf16, n):
    """Integers of the format's precision times 2^-10: every partial sum is an
    integer below 2^24 times 2^-10, exact in fp32, so the fold must be the
    float64 sum rounded once to the format (torch's cast: another code path).
    The sums need up to 17 (fp16) / 13 (bf16) bits, so the rounding works."""
    rng = np.random.default_rng(100 * n + bf16)
    top = 255 if bf16 else 2047
    tdt = torch.bfloat16 if bf16 else torch.float16
    ints = rng.integers(-top, top + 1, size=(n, 50_000))
    if n > 32:
        # n > 32 narrows between launches: keep the first 32's sum exact in the format
        ints[:32] = rng.integers(-3, 4, size=(32, 50_000))
    vals = ints.astype(np.float64) * 2.0 ** -10
    ins = [torch.from_numpy(v).to(tdt).view(torch.int16).numpy().view(np.uint16) for v in vals]
    for v, s in zip(vals, ins):   # the inputs themselves are exact in the format
        assert np.array_equal(torch.from_numpy(s.view(np.int16)).view(tdt).double().numpy(), v)
    want = torch.from_numpy(vals.sum(axis=0)).to(tdt).view(torch.int16).numpy().view(np.uint16)
    got = am.accum_fold(ins, bf16)
    assert np.array_equal(got, want)
    # the rounding had work to do: some sums are not representable in the format
    back = torch.from_numpy(want.view(np.int16)).view(tdt).double().numpy()
    assert (back != vals.sum(axis=0)).any()


# ---------------------------------------------------------- special values ----
# Each row: the sources of one element, and the expected bits, derived by hand
# from the contract in accum_model's docstring (not by running the model).

FP16_ROWS = [
    # NaN in the first source wins over a later one; payload and sign survive
    ((0x7E01, 0xFD55), 0x7E01),
    ((0xFD55, 0x7E01), 0xFF55),          # ... and a signalling first NaN is quieted
    ((0xFE03, 0x3C00, 0x7E01), 0xFE03),
    # a signalling NaN is quieted, wherever it stands
    ((0x7C01, 0x3C00), 0x7E01),
    ((0x3C00, 0x7C01), 0x7E01),
    ((0x3C00, 0x4000, 0xFC01), 0xFE01),
    # inf + -inf: the default NaN, sign set
    ((0x7C00, 0xFC00), 0xFE00),
    ((0xFC00, 0x7C00), 0xFE00),
    ((0x7C00, 0xFC00, 0x7E01), 0xFE00),  # the default NaN is then the first NaN
    # inf + finite
    ((0x7C00, 0xFBFF), 0x7C00),
    ((0xFC00, 0x7BFF), 0xFC00),
    # 65504 + 65504 overflows on narrowing; in fp32 it is finite
    ((0x7BFF, 0x7BFF), 0x7C00),
    ((0x7BFF, 0x7BFF, 0xFBFF), 0x7BFF),
    # subnormals are kept, in and out
    ((0x0001, 0x0001), 0x0002),
    ((0x83FF, 0x0001), 0x83FE),
    ((0x03FF, 0x0001), 0x0400),
    # signed zeros (RNE: -0 + +0 = +0)
    ((0x8000, 0x0000), 0x0000),
    ((0x0000, 0x8000), 0x0000),
    ((0x8000, 0x8000), 0x8000),
    # 65504, 1e-4, -65504: the small term is absorbed in fp32 (ulp 2^-8)
    ((0x7BFF, 0x068E, 0xFBFF), 0x0000),
    ((0x7BFF, 0xFBFF, 0x068E), 0x068E),  # another order keeps it
    # one narrowing: 1 + 2^-11 + 2^-11 = 1 + 2^-10 (per-add RNE would give 1)
    ((0x3C00, 0x1000), 0x3C00),
    ((0x3C01, 0x1000), 0x3C02),
    ((0x3C00, 0x1000, 0x1000), 0x3C01),
]

BF16_ROWS = [
    ((0x7FC1, 0xFFAA), 0x7FC1),
    ((0xFFAA, 0x7FC1), 0xFFEA),
    ((0xFFC3, 0x3F80, 0x7FC1), 0xFFC3),
    ((0x7F81, 0x3F80), 0x7FC1),
    ((0x3F80, 0x7F81), 0x7FC1),
    ((0x3F80, 0x4000, 0xFF81), 0xFFC1),
    ((0x7F80, 0xFF80), 0xFFC0),
    ((0xFF80, 0x7F80), 0xFFC0),
    ((0x7F80, 0xFF80, 0x7FC1), 0xFFC0),
    ((0x7F80, 0xFF7F), 0x7F80),
    ((0xFF80, 0x7F7F), 0xFF80),
    # 0x7f7f + 0x7f7f overflows fp32 itself: Inf, and it stays
    ((0x7F7F, 0x7F7F), 0x7F80),
    ((0x7F7F, 0x7F7F, 0xFF7F), 0x7F80),
    # max + half an ulp (2^119): finite in fp32, a tie that narrows to Inf
    ((0x7F7F, 0x7B00), 0x7F80),
    ((0x7F7F, 0x7B00, 0xFB00), 0x7F7F),
    ((0x0001, 0x0001), 0x0002),
    ((0x807F, 0x0001), 0x807E),
    ((0x007F, 0x0001), 0x0080),
    ((0x8000, 0x0000), 0x0000),
    ((0x0000, 0x8000), 0x0000),
    ((0x8000, 0x8000), 0x8000),
    # max, 1, -max: 1 is absorbed (fp32 ulp at 2^127 is 2^104)
    ((0x7F7F, 0x3F80, 0xFF7F), 0x0000),
    ((0x7F7F, 0xFF7F, 0x3F80), 0x3F80),
    # one narrowing: 1 + 2^-8 + 2^-8 = 1 + 2^-7
    ((0x3F80, 0x3B80), 0x3F80),
    ((0x3F81, 0x3B80), 0x3F82),
    ((0x3F80, 0x3B80, 0x3B80), 0x3F81),
]


@pytest.mark.parametrize("bf16,rows", [(False, FP16_ROWS), (True, BF16_ROWS)],
                         ids=["fp16", "bf16"])
def test_special_value_table(bf16, rows):
    for srcs, want in rows:
        got = am.accum_fold([u16(s) for s in srcs], bf16)
        assert got[0] == want, (f"{[hex(s) for s in srcs]}: got {int(got[0]):#06x}, "
                                f"want {want:#06x}")


@FORMATS
def test_one_source_is_a_byte_copy(bf16):
    h = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    assert np.array_equal(am.accum_fold([h], bf16), h)      # signalling NaNs untouched


def test_fold_bytes_trailing_byte_and_prefill():
    ins = [np.array([0x00, 0x3C, 0x11], np.uint8), np.array([0x00, 0x3C, 0x22], np.uint8)]
    assert am.fold_bytes(ins, 3, False).tolist() == [0x00, 0x40, 0x11]    # 1 + 1 = 2
    assert am.fold_bytes(ins, 0, False).tolist() == []
    assert am.fold_bytes(ins, 1, False).tolist() == [0x00]


# ------------------------------------------------------------ the inputs ----

@FORMATS
def test_cancel_is_deterministic_and_as_described(bf16):
    dt = DType.BFLOAT16 if bf16 else DType.FLOAT16
    a = am.cancel(dt, SMALL, 9, 5)
    b = am.cancel(dt, SMALL, 9, 5)
    c = am.cancel(dt, SMALL, 9, 6)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert any(not np.array_equal(x, y) for x, y in zip(a, c))
    m = np.stack(a)
    emask, one = (0x7F80, 0x3F80) if bf16 else (0x7C00, 0x3C00)
    assert bool(((m & emask) != emask).all())                 # finite
    mag = m & 0x7FFF
    big = mag > one                                           # |x| > 1: the pair only
    assert bool((big.sum(axis=0) == 2).all())
    lo, hi = ((127 + 20) << 7, (127 + 40) << 7) if bf16 else ((15 + 10) << 10, (15 + 15) << 10)
    assert bool(((mag[big] >= lo) & (mag[big] < hi)).all())
    # per element the two big entries are the same bits with the sign flipped
    order = np.argsort(~big, axis=0, kind="stable")[:2]
    first = np.take_along_axis(m, order[:1], axis=0)[0]
    second = np.take_along_axis(m, order[1:2], axis=0)[0]
    assert np.array_equal(first ^ 0x8000, second)
    # positions are spread over all the sources
    assert bool((big.sum(axis=1) > 0).all())


def _reverse(ins, bf16):
    return am.accum_fold(ins[::-1], bf16)


def _tree(ins, bf16):
    level = [am.up(s, bf16) for s in ins]
    while len(level) > 1:
        nxt = [am.add32(level[i], level[i + 1]) for i in range(0, len(level) - 1, 2)]
        if len(level) % 2:
            nxt.append(level[-1])
        level = nxt
    return am.down(level[0], bf16)


def _narrow_every_add(ins, bf16):
    """Reference mode's arithmetic: RNE to the format after every add."""
    acc = ins[0]
    for s in ins[1:]:
        acc = am.down(am.add32(am.up(acc, bf16), am.up(s, bf16)), bf16)
    return acc


def _down_trunc(x, bf16):
    """Narrowing by truncation (toward zero); finite inputs."""
    if bf16:
        return (x >> np.uint32(16)).astype(np.uint16)
    r = am.down(x, False)
    over = (am.up(r, False) & 0x7FFFFFFF) > (x & 0x7FFFFFFF)   # RNE went away from zero
    return np.where(over, r - np.uint16(1), r).astype(np.uint16)


def _truncating(ins, bf16):
    return am.accum_fold(ins, bf16, narrow=_down_trunc)


WRONG = {"reverse": _reverse, "tree": _tree, "narrow_every_add": _narrow_every_add,
         "truncating": _truncating}
# every source count tests/test_accum_gpu.py runs `cancel` inputs at
CANCEL_NS = [2, 3, 8, 9, 12, 16, 32, 40]


@FORMATS
@pytest.mark.parametrize("n", CANCEL_NS)
def test_cancel_inputs_tell_wrong_folds_apart(bf16, n):
    """A GPU pass on `cancel` inputs means something only if a wrong fold
    would have failed: at the small GPU shape each wrong fold differs from the
    model in at least 1 % of the elements (a floor, not a measurement).  For
    n = 3 the order variants may coincide with the model and are not required.
    For n = 2 there is one add and one narrowing, so the order variants and
    narrowing after every add ARE the model (asserted: equal); only truncation
    can differ."""
    dt = DType.BFLOAT16 if bf16 else DType.FLOAT16
    ins = am.cancel(dt, SMALL, n, 1)
    good = am.accum_fold(ins, bf16)
    shares = {name: float((fn(ins, bf16) != good).mean()) for name, fn in WRONG.items()}
    print(f"{'bf16' if bf16 else 'fp16'} n={n}: " +
          ", ".join(f"{k} {100 * v:.1f}%" for k, v in shares.items()))
    if n == 2:
        assert shares["reverse"] == 0 and shares["tree"] == 0 and shares["narrow_every_add"] == 0
        required = ["truncating"]
    elif n == 3:
        required = ["narrow_every_add", "truncating"]
    else:
        required = list(WRONG)
    for name in required:
        assert shares[name] >= 0.01, (name, shares)


@FORMATS
def test_cancel_inputs_tell_the_chain_from_one_long_fold(bf16):
    """n > 32 narrows between launches: on `cancel` inputs that differs from a
    single 40-source fp32 fold, so the GPU test of n = 40 pins the chain."""
    dt = DType.BFLOAT16 if bf16 else DType.FLOAT16
    ins = am.cancel(dt, SMALL, 40, 1)
    chained = am.accum_fold(ins, bf16)
    single = am.down(am.fold32(ins, bf16), bf16)
    share = float((chained != single).mean())
    print(f"{'bf16' if bf16 else 'fp16'} chain vs single fold: {100 * share:.1f}%")
    assert share >= 0.01
    # and the chain is what the docstring says: 32, then the running result + 8
    first = am.down(am.fold32(ins[:32], bf16), bf16)
    assert np.array_equal(chained, am.down(am.fold32([first] + ins[32:], bf16), bf16))


@FORMATS
def test_down_trunc_is_truncation(bf16):
    """The wrong narrowing used above really truncates: never away from zero,
    and less than one unit in the last place below."""
    rng = np.random.default_rng(3)
    e = rng.integers(127 - 20, 127 + 14, size=200_000, dtype=np.uint64)
    m = rng.integers(0, 1 << 23, size=200_000, dtype=np.uint64)
    x = ((e << 23) | m).astype(np.uint32)
    t = _down_trunc(x, bf16)
    lo = am.up(t, bf16).view(np.float32).astype(np.float64)
    hi = am.up(t + np.uint16(1), bf16).view(np.float32).astype(np.float64)
    v = x.view(np.float32).astype(np.float64)
    assert bool(((lo <= v) & (v < hi)).all())
