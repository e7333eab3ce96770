"""Stochastic-rounding compression on the host: the numpy definition
(prophet_amd/sr.py) against its stated properties, the compressors' host path,
the plan cache's key, host Worker rounds, and the C ABI's argument checks — no
GPU.  Every draw is a pure function of (key, step, element index), so the
statistical checks are deterministic."""
import ctypes

import numpy as np
import pytest

from prophet_amd import reducer, sr
from prophet_amd.compression import CastPlanCache, Compression
from prophet_amd.dtypes import DType
from prophet_amd.pushpull import ServerFrontend, Worker
from prophet_amd.reducer import SrKey

torch = pytest.importorskip("torch")

F32, F16, BF16 = int(DType.FLOAT32), int(DType.FLOAT16), int(DType.BFLOAT16)
ALL_R = np.arange(1 << 16, dtype=np.uint32)


def _f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32).copy()


def _bf16_f64(w):
    return (np.asarray(w, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def _fp16_f64(w):
    return np.asarray(w, np.uint16).view(np.float16).astype(np.float64)


def _over_all_r(fn, x):
    """fn over one value and every one of the 65,536 draws."""
    return fn(np.full(ALL_R.size, x, np.float32), ALL_R)


def _rtz_fp16(x):
    """Round-toward-zero fp16 bits of finite f32 values below 65536."""
    rne = torch.from_numpy(x).to(torch.float16).numpy()
    up = np.abs(rne.astype(np.float64)) > np.abs(x.astype(np.float64))
    return np.where(up, rne.view(np.uint16) - np.uint16(1), rne.view(np.uint16)).astype(np.uint16)


def test_philox_known_answers():
    for c0, c1, k, x0, x1 in [(0, 0, 0, 0xff1dae59, 0x6cd10df2),
                              (0xffffffff, 0xffffffff, 0xffffffff, 0x2c3f628b, 0xab4fd7ad),
                              (0x243f6a88, 0x85a308d3, 0x13198a2e, 0xdd7ce038, 0xf62a4c12)]:
        got = sr.philox2x32(c0, c1, k)
        assert (int(got[0]), int(got[1])) == (x0, x1)
    # arrays broadcast; the same answers element by element
    a, b = sr.philox2x32(np.array([0, 0xffffffff], np.uint32), np.array([0, 0xffffffff], np.uint32),
                         np.array([0, 0xffffffff], np.uint32))
    assert a.tolist() == [0xff1dae59, 0x2c3f628b] and b.tolist() == [0x6cd10df2, 0xab4fd7ad]


def test_bits_follow_the_element_index():
    """Element i takes 16 bits of philox(i >> 2, step, key): x0 low, x0 high,
    x1 low, x1 high; `first` shifts the index, nothing else."""
    key, step = 0x1234, 7
    r = sr.sr_bits(10, key, step)
    for i in range(10):
        x0, x1 = sr.philox2x32(i >> 2, step, key)
        word = int(x1 if i & 2 else x0)
        assert int(r[i]) == (word >> 16 if i & 1 else word & 0xffff)
    assert np.array_equal(sr.sr_bits(7, key, step, first=3), r[3:])
    big = (1 << 34) - 5
    tail = sr.sr_bits(5, key, step, first=big)
    x0, x1 = sr.philox2x32(0xffffffff, step, key)
    assert int(tail[-1]) == int(x1) >> 16 and int(tail[1]) == int(x0) & 0xffff
    with pytest.raises(ValueError):
        sr.sr_bits(6, key, step, first=big)                 # past 2^34 elements
    assert not np.array_equal(sr.sr_bits(64, key, step + 1), sr.sr_bits(64, key, step))
    assert not np.array_equal(sr.sr_bits(64, key + 1, step), sr.sr_bits(64, key, step))


def _specials():
    """The g list of tests/test_compress_ef_gpu.py:_specials."""
    return _f32([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007fffff, 0x00008000,
                 0x00008001, 0x00800000,
                 0x3f800fff, 0x3f801000, 0x3f801001, 0x3f802fff, 0x3f803000, 0x3f803001,
                 0x33000000, 0x33000001, 0x33800000, 0x33c00000, 0x32ffffff,
                 0x3f807fff, 0x3f808000, 0x3f808001, 0x3f817fff, 0x3f818000, 0x3f818001,
                 0x477fdfff, 0x477fe000, 0xc77fdfff, 0xc77fe000, 0x7f7f7fff, 0x7f7f8000,
                 0xff7f8000, 0x7f7fffff, 0xff7fffff,
                 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00001, 0x7f800001])


def _random(n=400_000, seed=5):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * np.exp2(rng.integers(90, 145, n) - 127.0)
    return x.astype(np.float32)


def test_bf16_properties():
    x = np.concatenate([_random(), _specials()])
    u = x.view(np.uint32)
    fin = (u & 0x7f800000) != 0x7f800000
    zero, ones = np.zeros(x.size, np.uint32), np.full(x.size, 0xffff, np.uint32)
    lo, hi = sr.sr_bf16(x, zero), sr.sr_bf16(x, ones)
    # r16 = 0 truncates; r16 = 0xffff moves by one step unless the value is exact
    assert np.array_equal(lo[fin], (u[fin] >> 16).astype(np.uint16))
    exact = (u & 0xffff) == 0
    assert np.array_equal(hi[fin & exact], lo[fin & exact])
    assert np.array_equal(hi[fin & ~exact], (lo[fin & ~exact] + 1).astype(np.uint16))
    # inf stays inf, a NaN a NaN, whatever the draw
    for w in (lo, hi):
        f = _bf16_f64(w)
        assert np.array_equal(np.isnan(f), np.isnan(x)) and np.array_equal(np.isinf(f[~fin]),
                                                                           np.isinf(x[~fin]))
        assert np.array_equal(f[np.isinf(x)], x[np.isinf(x)].astype(np.float64))
    # subnormals and signed zeros are kept, bit for bit, where bf16 holds them
    for bits in (0x00000000, 0x80000000, 0x00010000, 0x80010000, 0x007f0000):
        assert (_over_all_r(sr.sr_bf16, _f32([bits])[0]) == bits >> 16).all()
    # the mean over all draws is exactly g
    for g in (np.float32(1 + 2.0 ** -12), np.float32(3e-6), np.float32(1e-8), _f32([0x00008001])[0],
              np.float32(-1234.567)):
        assert _bf16_f64(_over_all_r(sr.sr_bf16, g)).mean() == float(g), g
    # a finite value above bf16's largest goes to inf as often as its position says
    big = np.float32(3.4e38)
    frac = (int(big.view(np.uint32)) & 0xffff) / 65536.0
    got = np.isinf(_bf16_f64(_over_all_r(sr.sr_bf16, big))).mean()
    assert got == frac and 0.78 < got < 0.80
    assert np.isfinite(_bf16_f64(_over_all_r(sr.sr_bf16, _f32([0x7f7f0000])[0]))).all()


def test_fp16_properties():
    x = np.concatenate([_random(), _specials()])
    u = x.view(np.uint32)
    a = u & 0x7fffffff
    fin = (u & 0x7f800000) != 0x7f800000
    small = a < 0x47800000                                   # |x| < 65536
    zero, ones = np.zeros(x.size, np.uint32), np.full(x.size, 0xffff, np.uint32)
    lo, hi = sr.sr_fp16(x, zero), sr.sr_fp16(x, ones)
    assert np.array_equal(lo[small], _rtz_fp16(x[small]))    # r16 = 0: round toward zero
    step = hi[small].astype(np.int64) - lo[small].astype(np.int64)
    assert set(np.unique(step)) <= {0, 1}
    exact = _fp16_f64(lo[small]) == x[small].astype(np.float64)
    assert (step[exact] == 0).all()
    # |x| >= 65536: inf of the value's sign; inf and NaN as the plain cast
    for w in (lo, hi):
        f = _fp16_f64(w)
        assert np.array_equal(f[fin & ~small], np.sign(x[fin & ~small]) * np.inf)
        assert np.array_equal(np.isnan(f), np.isnan(x))
        assert np.array_equal(f[np.isinf(x)], x[np.isinf(x)].astype(np.float64))
    assert (_over_all_r(sr.sr_fp16, np.float32(-0.0)) == 0x8000).all()
    # the mean over all draws: exact in the normal range and where 16 bits hold
    # the dropped fraction, short by at most 2^-16 of a subnormal step elsewhere
    for g in (np.float32(1 + 2.0 ** -14), np.float32(3e-6)):
        assert _fp16_f64(_over_all_r(sr.sr_fp16, g)).mean() == float(g), g
    m = _fp16_f64(_over_all_r(sr.sr_fp16, np.float32(1e-8))).mean()
    assert 0 <= float(np.float32(1e-8)) - m <= 2.0 ** -40
    assert abs(m - 9.99989e-9) < 1e-14
    # 65520 is halfway between fp16's largest and 65536
    assert np.isinf(_fp16_f64(_over_all_r(sr.sr_fp16, np.float32(65520.0)))).mean() == 0.5
    # below 2^-40 * 2^-24 nothing is ever delivered
    assert (_over_all_r(sr.sr_fp16, np.float32(2.0 ** -66)) == 0).all()


def test_specials_table():
    """Every special value under r16 = 0, 0x8000 and 0xffff, against the rule
    stated independently: the two neighbours in the wire format and the carry
    out of (dropped fraction + r16)."""
    g = _specials()
    fin = np.isfinite(g)
    for r in (0, 0x8000, 0xffff):
        rr = np.full(g.size, r, np.uint32)
        b, h = sr.sr_bf16(g, rr), sr.sr_fp16(g, rr)
        for i in np.flatnonzero(fin):
            u = int(g[i].view(np.uint32))
            assert int(b[i]) == ((u >> 16) + (((u & 0xffff) + r) >> 16)), hex(u)
            x = abs(float(g[i]))
            sign = 0x8000 if u >> 31 else 0
            if x >= 65536.0:
                assert int(h[i]) == sign | 0x7c00, hex(u)
                continue
            down = int(_rtz_fp16(np.array([x], np.float32))[0])
            ulp = 2.0 ** -24 if down < 0x400 else 2.0 ** ((down >> 10) - 25)
            frac = int((x - float(np.uint16(down).view(np.float16))) / ulp * 65536.0)   # floor
            assert int(h[i]) == sign | (down + ((frac + r) >> 16)), hex(u)
        for w, to in ((b, _bf16_f64), (h, _fp16_f64)):
            f = to(w)
            assert np.array_equal(np.isnan(f), np.isnan(g))
            assert np.array_equal(f[np.isinf(g)], g[np.isinf(g)].astype(np.float64))


def test_unbiased_at_fixed_seeds():
    """4,096 elements x 256 steps under key 0x1234: the mean of the delivered
    values lies within 6 standard errors of g under the binomial model (one
    wire step times sqrt(p (1 - p) / N), p the dropped fraction), where the
    plain cast delivers a constant."""
    n, steps, key = 4096, 256, 0x1234
    N = n * steps
    # bf16: 1 + 2^-12, step 2^-7, p = 2^-5; plain bf16 gives exactly 1.0
    g = np.float32(1 + 2.0 ** -12)
    x = np.full(n, g, np.float32)
    tot = sum(_bf16_f64(sr.sr_round(x, key, s, "bf16")).sum() for s in range(steps))
    p = 2.0 ** -5
    se = 2.0 ** -7 * np.sqrt(p * (1 - p) / N)
    assert abs(tot / N - float(g)) <= 6 * se
    assert abs(tot / N - 1.00024201) < 5e-9                  # the recorded outcome
    assert float(torch.tensor([float(g)]).to(torch.bfloat16).float()) == 1.0
    # fp16: 1e-8, step 2^-24, p = 1e-8 / 2^-24; plain fp16 gives exactly 0
    g = np.float32(1e-8)
    x = np.full(n, g, np.float32)
    tot = sum(_fp16_f64(sr.sr_round(x, key, s, "fp16")).sum() for s in range(steps))
    p = float(g) / 2.0 ** -24
    se = 2.0 ** -24 * np.sqrt(p * (1 - p) / N)
    assert abs(tot / N - float(g)) <= 6 * se
    assert tot > 0 and float(torch.tensor([1e-8]).to(torch.float16).float()) == 0.0


WIRES = [(Compression.fp16_sr, Compression.fp16, "fp16", np.float16),
         (Compression.bf16_sr, Compression.bf16, "bf16", np.uint16)]


@pytest.mark.parametrize("kind", ["torch", "numpy"])
@pytest.mark.parametrize("comp,plain,name,npdt", WIRES)
def test_compressors_on_the_host(comp, plain, name, npdt, kind):
    x = np.concatenate([_random(5000, seed=9), _specials()])
    t = torch.from_numpy(x) if kind == "torch" else x
    assert comp.STOCHASTIC and not comp.ERROR_FEEDBACK and not plain.STOCHASTIC
    assert issubclass(comp, plain) and comp.WIRE_DTYPE == plain.WIRE_DTYPE
    out = comp.wire_like(t)
    assert comp.compress_sr_into(out, t, 0xdeadbeef, 5) is out
    bits = (out.view(torch.int16).numpy().view(np.uint16) if kind == "torch"
            else out.view(np.uint16))
    assert np.array_equal(bits, sr.sr_round(x, 0xdeadbeef, 5, name))
    again = comp.wire_like(t)
    comp.compress_sr_into(again, t, 0xdeadbeef, 5)
    other = comp.wire_like(t)
    comp.compress_sr_into(other, t, 0xdeadbeef, 6)
    as_bits = (lambda o: o.view(torch.int16).numpy() if kind == "torch" else o.view(np.uint16))
    assert np.array_equal(as_bits(again), as_bits(out))
    assert not np.array_equal(as_bits(other), as_bits(out))
    # key and step are taken mod 2^32
    comp.compress_sr_into(again, t, 0xdeadbeef + (1 << 32), 5 + (1 << 32))
    assert np.array_equal(as_bits(again), as_bits(out))
    # the stateless compress stays the plain cast; decompress is inherited
    c, ctx = comp.compress(t)
    pc, _ = plain.compress(t)
    assert np.array_equal(as_bits(c), as_bits(pc))
    back = comp.decompress(out, ctx)
    want = plain.decompress(out, ctx)
    assert np.array_equal(np.asarray(back).view(np.uint32), np.asarray(want).view(np.uint32))
    # float32 only
    assert comp.compresses(t)
    for other_dt in (np.float64, np.float16, np.int32):
        y = np.ones(8, other_dt) if kind == "numpy" else torch.from_numpy(np.ones(8, other_dt))
        assert not comp.compresses(y)
        with pytest.raises(ValueError):
            comp.compress_sr_into(comp.wire_like(y), y, 1, 1)
    # many: one by one on the host
    parts = [t[:300], t[300:1000]]
    outs = [comp.wire_like(p) for p in parts]
    comp.compress_many_sr_into(outs, parts, [11, 12], 3)
    for o, p, k in zip(outs, parts, (11, 12)):
        assert np.array_equal(np.asarray(as_bits(o)).view(np.uint16),
                              sr.sr_round(np.asarray(p), k, 3, name))
    with pytest.raises(ValueError):
        comp.compress_many_sr_into(outs, parts, [11], 3)


def test_plan_cache_key_carries_the_keys(monkeypatch):
    import prophet_amd.compression as comp

    class T:
        def __init__(self, p, n=8):
            self.p, self.n = p, n

        def data_ptr(self):
            return self.p

        def numel(self):
            return self.n

    class P:
        def close(self):
            pass

    made = []
    monkeypatch.setattr(comp, "_new_plan", lambda dt, pairs, wire=2: made.append(
        [tuple(p[2:]) for p in pairs]) or P())
    c = CastPlanCache(4)
    w, h = T(0x1000), T(0x2000)
    a = c.get(F32, [(w, h)])
    b = c.get(F32, [(w, h, SrKey(7))])
    assert b is not a and c.built == 2                       # an SR plan is another plan
    assert c.get(F32, [(w, h, SrKey(7))]) is b and c.built == 2          # hit
    assert c.get(F32, [(w, h, SrKey(8))]) is not b and c.built == 3      # another key misses
    assert c.get(F32, [(w, h)]) is a and c.built == 3
    # a residual at an address equal to a key's value is still another plan
    assert c.get(F32, [(w, h, T(7))]) is not b and c.built == 4
    assert made[1] == [(SrKey(7),)] and isinstance(made[1][0][0], SrKey)
    c.close()


class LastPushServer:
    """One worker's host server: a pull returns the key's last push."""

    def __init__(self):
        self.store = {}
        self.dtypes = {}

    def push(self, key, worker, data, dtype, nbytes=None):
        self.store[key] = np.asarray(data).view(np.uint8).copy()
        self.dtypes[key] = int(dtype)

    def pull(self, key, out, nbytes=None):
        np.asarray(out).view(np.uint8)[:] = self.store[key]


def test_worker_rounds_on_the_host():
    """The step advances by one per compress call, the key is x0 of
    philox(declared key, rank, seed), two ranks (and two seeds) draw different
    bits, and the delivered bytes are the definition's."""
    n = 1000
    g = _random(n, seed=11)

    def worker(rank, seed=0):
        w = Worker(rank, ServerFrontend(LastPushServer(), size=1), sr_seed=seed)
        w.declare("pad")
        w.declare("g")
        w.init_tensor("pad", np.zeros(4, np.float32), DType.FLOAT32)
        ctx = w.init_tensor("g", g.copy(), DType.FLOAT32, compression=Compression.bf16_sr)
        assert ctx.dtype == DType.BFLOAT16 and ctx.size == 2 * n and ctx.residual is None
        # the init push is the plain cast and uses no step
        assert np.array_equal(ctx.staging, torch.from_numpy(g).to(torch.bfloat16)
                              .view(torch.int16).numpy().view(np.uint16))
        assert w.sr_step == 0
        return w, ctx

    w0, c0 = worker(0)
    w1, c1 = worker(1)
    w2, c2 = worker(0, seed=99)
    assert c0.sr_key == int(sr.philox2x32(1, 0, 0)[0]) == sr.context_key(1, 0, 0)
    assert c1.sr_key == int(sr.philox2x32(1, 1, 0)[0])
    assert c2.sr_key == int(sr.philox2x32(1, 0, 99)[0])
    assert len({c0.sr_key, c1.sr_key, c2.sr_key}) == 3
    outs = []
    for w, c in ((w0, c0), (w1, c1), (w2, c2)):
        for step in range(3):
            x = g.copy()
            w.push_pull("g", x)
            assert w.sr_step == step + 1
            want = sr.sr_round(g, c.sr_key, step, "bf16")
            assert np.array_equal(c.staging, want)
            assert np.array_equal(x.view(np.uint32), want.astype(np.uint32) << 16)
        outs.append(c.staging.copy())
        with pytest.raises(ValueError):
            w.broadcast("g", g.copy(), root_rank=0)
    assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[0], outs[2])
    # the async form takes steps from the same counter
    h = w0.push_pull_async("g", g.copy())
    w0.synchronize(h)
    assert w0.sr_step == 4
    # a plain push_pull on an uncompressed context uses none
    w0.push_pull("pad", np.ones(4, np.float32))
    assert w0.sr_step == 4
    for w in (w0, w1, w2):
        w.close()
    # f64 under an SR compressor passes through uncompressed
    w = Worker(0, ServerFrontend(LastPushServer(), size=1))
    w.declare("f64")
    ctx = w.init_tensor("f64", np.zeros(8, np.float64), DType.FLOAT64,
                        compression=Compression.fp16_sr)
    assert ctx.compressor is None and ctx.dtype == DType.FLOAT64


def test_worker_iteration_mixes_compressors_on_the_host():
    """push_pull_iteration over all seven compressors equals per-tensor
    push_pull except in the steps it uses: one per SR compressor and
    iteration, every context of it under its own key."""
    n = 64
    names = ["none", "fp16", "bf16", "fp16_ef", "bf16_ef", "fp16_sr", "bf16_sr", "bf16_sr2"]
    comps = [getattr(Compression, k.rstrip("2")) for k in names]
    g = _random(n * len(names), seed=13)
    g = np.where(np.abs(g) < 6e4, g, np.float32(1.5)).astype(np.float32)

    def worker():
        w = Worker(3, ServerFrontend(LastPushServer(), size=1), sr_seed=42)
        for k in names:
            w.declare(k)
        for i, (k, comp) in enumerate(zip(names, comps)):
            w.init_tensor(k, g[i * n:(i + 1) * n].copy(), DType.FLOAT32, compression=comp)
        return w

    w1, w2 = worker(), worker()
    for it in range(3):
        x1 = {k: (g[i * n:(i + 1) * n] * np.float32(1 + it)).copy() for i, k in enumerate(names)}
        x2 = {k: v.copy() for k, v in x1.items()}
        src = {k: v.copy() for k, v in x1.items()}
        for k in names:
            w1.push_pull(k, x1[k])
        w2.push_pull_iteration(x2)
        assert w1.sr_step == 3 * (it + 1) and w2.sr_step == 2 * (it + 1)
        for k in names[:5]:                                   # no SR: the same bytes
            assert np.array_equal(x1[k].view(np.uint32), x2[k].view(np.uint32)), (it, k)
        # fp16_sr is the iteration's first SR launch, the two bf16_sr contexts share the second
        for k, wire, step in (("fp16_sr", "fp16", 2 * it), ("bf16_sr", "bf16", 2 * it + 1),
                              ("bf16_sr2", "bf16", 2 * it + 1)):
            c = w2.contexts[k]
            assert c.sr_key == sr.context_key(c.declared_key, 3, 42)
            assert np.array_equal(c.staging.view(np.uint16),
                                  sr.sr_round(src[k], c.sr_key, step, wire)), (it, k)
            back = c.compressor.decompress(c.staging, np.dtype(np.float32))
            assert np.array_equal(x2[k].view(np.uint32), back.view(np.uint32))
        assert w2.contexts["bf16_sr"].sr_key != w2.contexts["bf16_sr2"].sr_key
    assert len(w2._cast_plans) == 0                           # host tensors build no plan
    w1.close()
    w2.close()


# ------------------------------------------------------------- C ABI checks --
A, B, C, D, E = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000


@pytest.fixture(scope="module")
def lib():
    return reducer.load_library()


def test_compress_sr_argument_errors_without_a_gpu(lib):
    f = lib.byteps_reduce_compress_sr
    for dt in (DType.FLOAT64, DType.FLOAT16, DType.BFLOAT16, DType.INT32, DType.UINT8, 7, -1):
        for wire in (F16, BF16):
            assert f(A, B, 64, int(dt), wire, 1, 2, None) == reducer.EDTYPE, (dt, wire)
            assert b"data type" in lib.byteps_reduce_last_error()
    for wire in (F32, int(DType.FLOAT64), int(DType.INT32), 7, -1):
        assert f(A, B, 64, F32, wire, 1, 2, None) == reducer.EDTYPE, wire
    for wire in (F16, BF16):
        assert f(None, B, 64, F32, wire, 1, 2, None) == reducer.EARGS
        assert f(A, None, 64, F32, wire, 1, 2, None) == reducer.EARGS
        assert b"null" in lib.byteps_reduce_last_error()
        assert f(A, A, 64, F32, wire, 1, 2, None) == reducer.EARGS
        assert f(A, A + 127, 64, F32, wire, 1, 2, None) == reducer.EARGS     # dst 128 bytes
        assert f(B + 255, B, 64, F32, wire, 1, 2, None) == reducer.EARGS     # src 256 bytes
        assert b"overlap" in lib.byteps_reduce_last_error()
        assert f(None, None, 0, F32, wire, 1, 2, None) == reducer.OK         # nothing to do
        assert f(A, 1 << 40, (1 << 34) + 1, F32, wire, 1, 2, None) == reducer.EARGS
        assert b"2^34" in lib.byteps_reduce_last_error()
    assert lib.byteps_reduce_version() == 5


def _segs(*quads):
    arr = (reducer.CastSrDesc * max(1, len(quads)))()
    for i, (w, h, n, k) in enumerate(quads):
        arr[i].wide, arr[i].half, arr[i].nelem, arr[i].key = w, h, n, k
    return arr


def test_sr_plan_argument_errors_without_a_gpu(lib):
    def create(quads, dt, wire, nsegs=None):
        out = ctypes.c_void_p(0x1234)
        rc = lib.byteps_reduce_cast_plan_create_sr(
            _segs(*quads), len(quads) if nsegs is None else nsegs, int(dt), int(wire),
            ctypes.byref(out))
        return rc, out

    assert ctypes.sizeof(reducer.CastSrDesc) == 32
    for dt, wire in [(DType.FLOAT64, F16), (DType.BFLOAT16, F16), (DType.FLOAT16, BF16),
                     (DType.INT32, BF16), (7, F16), (F32, F32), (F32, -1)]:
        rc, out = create([(A, B, 64, 1)], dt, wire)
        assert rc == reducer.EDTYPE and not out.value, (dt, wire)
        assert b"data type" in lib.byteps_reduce_last_error()
    for wire in (F16, BF16):
        assert create([(A, B, 64, 1), (None, E, 8, 2)], F32, wire)[0] == reducer.EARGS
        assert create([(A, B, 64, 1), (D, None, 8, 2)], F32, wire)[0] == reducer.EARGS
        assert create([(A, B, 64, 1)], F32, wire, nsegs=-1)[0] == reducer.EARGS
        assert lib.byteps_reduce_cast_plan_create_sr(
            None, 2, F32, wire, ctypes.byref(ctypes.c_void_p())) == reducer.EARGS
        assert lib.byteps_reduce_cast_plan_create_sr(_segs((A, B, 64, 1)), 1, F32, wire,
                                                     None) == reducer.EARGS
        for bad in ([(A, A + 396, 100, 1)], [(A, B, 100, 1), (A + 396, E, 100, 2)],
                    [(A, B, 100, 1), (D, B + 198, 100, 2)], [(A, B, 100, 1), (B, E, 100, 1)]):
            assert create(bad, F32, wire)[0] == reducer.EARGS, bad
            assert b"overlap" in lib.byteps_reduce_last_error()
        rc, out = create([(1 << 40, 1 << 41, (1 << 34) + 1, 1)], F32, wire)
        assert rc == reducer.EARGS and b"2^34" in lib.byteps_reduce_last_error()
    assert lib.byteps_reduce_cast_plan_compress_sr(None, 0, None) == reducer.EARGS


def test_reducer_surface_without_a_gpu(monkeypatch):
    red = reducer.GpuReducer()
    called = []
    for name in ("byteps_reduce_compress_sr", "byteps_reduce_cast_plan_create_sr"):
        monkeypatch.setattr(red.lib, name,
                            lambda *a, name=name: called.append((name, a)) or reducer.EARGS)
    wire = torch.empty(100, dtype=torch.bfloat16)
    wide = torch.empty(100, dtype=torch.float32)
    with pytest.raises(ValueError):
        red.compress_sr(wire[:99], wide, 100, 1, 2, DType.BFLOAT16)
    with pytest.raises(ValueError):
        red.compress_sr(wire, wide[:99], 100, 1, 2, DType.BFLOAT16)
    with pytest.raises(ValueError):
        red.cast_plan([(wide, wire[:99], 100, SrKey(1))], DType.FLOAT32, DType.BFLOAT16)
    with pytest.raises(ValueError):                                 # keys: all or none
        red.cast_plan([(wide, wire, 100, SrKey(1)), (wide, wire, 100)], DType.FLOAT32,
                      DType.BFLOAT16)
    assert not called
    with pytest.raises(reducer.ReduceError):
        red.compress_sr(wire, wide, 100, (1 << 32) + 5, -1, DType.BFLOAT16)
    assert called[0][1][5:7] == (5, 0xffffffff)                     # key, step mod 2^32
    with pytest.raises(reducer.ReduceError):
        red.cast_plan([(wide, wire, 100, SrKey(9))], DType.FLOAT32, DType.BFLOAT16)
    assert [c[0] for c in called] == ["byteps_reduce_compress_sr",
                                      "byteps_reduce_cast_plan_create_sr"]


def test_ops_are_registered_and_mutate_dst():
    from prophet_amd import torch_ops
    for name in ("compress_fp16_sr_out", "compress_bf16_sr_out"):
        assert name in torch_ops.OPS
        s = str(getattr(torch.ops.bpsr, name).default._schema)
        assert "Tensor(a0!) dst" in s and "Tensor src" in s and " key" in s and " step" in s
        assert "(a1!)" not in s
        with pytest.raises(NotImplementedError):                   # no CPU kernel
            getattr(torch.ops.bpsr, name)(torch.empty(4, dtype=torch.float16), torch.ones(4), 1, 2)
