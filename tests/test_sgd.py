"""The SGD step inside the decompress on the host: the numpy definition
(prophet_amd/sgd.py) against torch.optim.SGD on inputs whose every product and
sum is exact, hand-computed subnormal products, the divide, the compressors'
host path of ``apply_sgd_many`` and the argument errors raised in Python — no
GPU."""
import numpy as np
import pytest

from prophet_amd import sgd
from prophet_amd.compression import CastPlanCache, ClipValues, Compression

torch = pytest.importorskip("torch")

WIRE_OF = {"fp16": Compression.fp16, "bf16": Compression.bf16}


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def _wire_bits(values, wire):
    """float values (exact in the wire format) as uint16 wire bits."""
    t = torch.tensor(np.asarray(values, np.float32))
    t = t.to(torch.float16 if wire == "fp16" else torch.bfloat16)
    assert torch.equal(t.float(), torch.tensor(np.asarray(values, np.float32))), "exact on the wire"
    return t.view(torch.int16).numpy().view(np.uint16).copy()


def _exact_inputs(n, seed):
    """Small integers times powers of two, gradients never zero: with lr, mu
    and wd powers of two every product and sum of three steps is exact."""
    rng = np.random.default_rng(seed)
    p = (rng.integers(-8, 9, n) * np.exp2(rng.integers(-2, 3, n))).astype(np.float32)
    gs = []
    for _ in range(3):
        m = rng.integers(1, 9, n) * rng.choice([-1, 1], n)
        gs.append((m * np.exp2(rng.integers(-2, 3, n))).astype(np.float32))
    return p, gs


@pytest.mark.parametrize("nesterov", [False, True], ids=["plain", "nesterov"])
@pytest.mark.parametrize("wd", [0.0, 2.0 ** -4], ids=["nowd", "wd"])
@pytest.mark.parametrize("mu", [0.0, 0.5], ids=["mu0", "mu.5"])
@pytest.mark.parametrize("wire", ["fp16", "bf16"])
def test_definition_is_torch_sgd_on_exact_inputs(wire, mu, wd, nesterov):
    if nesterov and mu == 0.0:
        with pytest.raises(ValueError):
            sgd.check_hyper(0.125, mu, wd, nesterov)
        return
    lr = 2.0 ** -3
    p0, gs = _exact_inputs(257, 11)
    tp = torch.nn.Parameter(torch.tensor(p0.copy()))
    opt = torch.optim.SGD([tp], lr=lr, momentum=mu, weight_decay=wd, nesterov=nesterov,
                          foreach=False)
    p, m = p0.copy(), np.zeros_like(p0)
    for g in gs:
        tp.grad = torch.tensor(g.copy())
        opt.step()
        p, m = sgd.sgd_step(p, m, _wire_bits(g, wire), wire, lr=lr, momentum=mu,
                            weight_decay=wd, nesterov=nesterov)
        assert np.array_equal(p, tp.detach().numpy()), "equal values after each step"
        if mu:
            buf = opt.state[tp]["momentum_buffer"].numpy()
            assert np.array_equal(m, buf)


def test_subnormal_products_are_kept_not_flushed():
    """lr * d and wd * p below 2^-126, computed by hand."""
    f = np.float32
    # wd * p = 2^-10 * 2^-120 = 2^-130 (subnormal); g = 2^-128 (bf16 holds it)
    # g + wd*p = 2^-128 + 2^-130 = 5 * 2^-130; mu = 0: m' = that; d = m'
    # lr * d = 2^-3 * 5 * 2^-130 = 5 * 2^-133 (subnormal, exact: 2^-149 * 5 * 2^16)
    # p' = 2^-120 - 5 * 2^-133 = 2^-133 * (2^13 - 5), exact
    p = np.array([2.0 ** -120], f)
    h = _wire_bits([2.0 ** -128], "bf16")
    pn, mn = sgd.sgd_step(p, np.zeros(1, f), h, "bf16", lr=2.0 ** -3, weight_decay=2.0 ** -10)
    assert float(mn[0]) == 5 * 2.0 ** -130 and mn[0] != 0
    assert float(pn[0]) == 2.0 ** -133 * (2 ** 13 - 5)
    # flushed, wd * p would be 0 and m' = 2^-128 (itself flushed: 0)
    assert _bits(mn)[0] == 5 << 19                 # 5 * 2^-130 = 5 * 2^19 * 2^-149
    # a subnormal lr * d alone: g = 2^-24 (the smallest fp16 subnormal), lr = 2^-110
    p = np.array([0.0], f)
    pn, mn = sgd.sgd_step(p, np.zeros(1, f), np.array([1], np.uint16), "fp16", lr=2.0 ** -110)
    assert float(mn[0]) == 2.0 ** -24
    assert float(pn[0]) == -(2.0 ** -134) and _bits(pn)[0] == 0x80000000 | (1 << 15)
    # mult makes a subnormal gradient: 2^-14 * 2^-120
    pn, mn = sgd.sgd_step(p, np.zeros(1, f), _wire_bits([2.0 ** -14], "fp16"), "fp16", lr=1.0,
                          mult=f(2.0 ** -120))
    assert float(mn[0]) == 2.0 ** -134 and float(pn[0]) == -(2.0 ** -134)


@pytest.mark.parametrize("wire", ["fp16", "bf16"])
def test_divisor_is_the_host_decompress_divide(wire):
    """divisor 8: the host decompress_into(divisor=8) value, fed (it is exact
    on the wire) into the divisor-1 definition."""
    comp = WIRE_OF[wire]
    bits = np.arange(1 << 16, dtype=np.uint16)
    wt = torch.from_numpy(bits.view(np.int16)).view(comp.wire_torch_dtype())
    out = torch.empty(bits.size, dtype=torch.float32)
    comp.decompress_into(out, wt, divisor=8)
    g8 = sgd.wire_to_f32(bits, wire, 8)
    nan = np.isnan(out.numpy())
    assert np.array_equal(np.isnan(g8), nan)
    assert np.array_equal(_bits(g8)[~nan], _bits(out.numpy())[~nan])
    rng = np.random.default_rng(3)
    p = rng.standard_normal(bits.size).astype(np.float32)
    m = rng.standard_normal(bits.size).astype(np.float32)
    back = out.to(comp.wire_torch_dtype())
    assert torch.equal(back.float()[~torch.from_numpy(nan)], out[~torch.from_numpy(nan)])
    hb = back.view(torch.int16).numpy().view(np.uint16)
    kw = dict(lr=0.1, momentum=0.9, weight_decay=1e-4, nesterov=True)
    a = sgd.sgd_step(p, m, bits, wire, 8, **kw)
    b = sgd.sgd_step(p, m, hb, wire, 1, **kw)
    for x, y in zip(a, b):
        assert np.array_equal(np.isnan(x), np.isnan(y))
        assert np.array_equal(_bits(x)[~np.isnan(x)], _bits(y)[~np.isnan(y)])


def _host_case(wire, kind, n=1000, seed=5):
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 10, n))).astype(np.float32)
    m = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 10, n))).astype(np.float32)
    g = (rng.standard_normal(n) * np.exp2(rng.integers(-10, 6, n))).astype(np.float32)
    h = torch.tensor(g).to(torch.float16 if wire == "fp16" else torch.bfloat16)
    if kind == "torch":
        return torch.tensor(p), h, torch.tensor(m)
    hb = h.view(torch.int16).numpy().view(np.uint16).copy()
    return p, (hb.view(np.float16) if wire == "fp16" else hb), m


def _np(x):
    return x.numpy() if hasattr(x, "data_ptr") else x


def _hbits(h):
    if hasattr(h, "data_ptr"):
        return h.view(torch.int16).numpy().view(np.uint16)
    return h.view(np.uint16)


@pytest.mark.parametrize("kind", ["numpy", "torch"])
@pytest.mark.parametrize("wire", ["fp16", "bf16"])
def test_host_path_of_apply_sgd_many_is_the_definition(wire, kind):
    comp = WIRE_OF[wire]
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
    for record in (None, ClipValues(1.0, 0.0, 1.0, np.float32(0.7), np.float32(0.7 * 2.0 ** -7))):
        cases = [_host_case(wire, kind, n, 5 + n) for n in (1000, 1, 8)]
        want = [sgd.sgd_step(_np(p).copy(), _np(m).copy(), _hbits(h).copy(), wire, 8,
                             mult=None if record is None else record.mult, **kw)
                for p, h, m in cases]
        wires = [_hbits(h).copy() for _, h, _ in cases]
        got = comp.apply_sgd_many([c[0] for c in cases], [c[1] for c in cases],
                                  [c[2] for c in cases], 8, record=record,
                                  skip_nonfinite=record is not None, **kw)
        assert got[0] is cases[0][0]
        for (p, h, m), (pn, mn), w in zip(cases, want, wires):
            assert np.array_equal(_bits(_np(p)), _bits(pn))
            assert np.array_equal(_bits(_np(m)), _bits(mn))
            assert np.array_equal(_hbits(h), w), "the wire is read only"
    # the one-tensor form
    p, h, m = _host_case(wire, kind, 77, 9)
    pn, mn = sgd.sgd_step(_np(p).copy(), _np(m).copy(), _hbits(h).copy(), wire, 1, lr=0.5)
    assert comp.apply_sgd_into(p, h, m, lr=0.5) is p
    assert np.array_equal(_bits(_np(p)), _bits(pn)) and np.array_equal(_bits(_np(m)), _bits(mn))


@pytest.mark.parametrize("wire", ["fp16", "bf16"])
def test_host_skip_leaves_every_byte(wire):
    comp = WIRE_OF[wire]
    kw = dict(lr=0.05, momentum=0.9)
    p, h, m = _host_case(wire, "numpy")
    p0, m0 = p.copy(), m.copy()
    found = ClipValues(1.0, 1.0, 1.0, np.float32(1.0), np.float32(0.5))
    comp.apply_sgd_many([p], [h], [m], record=found, skip_nonfinite=True, **kw)
    assert np.array_equal(_bits(p), _bits(p0)) and np.array_equal(_bits(m), _bits(m0))
    # the same record without the skip, and a clean record with it: applied
    for rec, skip in ((found, False), (ClipValues(1.0, 0.0, 1.0, np.float32(1.0),
                                                  np.float32(0.5)), True)):
        p, m = p0.copy(), m0.copy()
        pn, mn = sgd.sgd_step(p0, m0, _hbits(h), wire, mult=np.float32(0.5), **kw)
        comp.apply_sgd_many([p], [h], [m], record=rec, skip_nonfinite=skip, **kw)
        assert np.array_equal(_bits(p), _bits(pn)) and np.array_equal(_bits(m), _bits(mn))
        assert not np.array_equal(_bits(p), _bits(p0))


def test_argument_errors_raised_in_python():
    comp = Compression.fp16
    p, h, m = _host_case("fp16", "numpy", 16)
    ok = dict(lr=0.1)
    bad = [dict(lr=float("inf")), dict(lr=float("nan")), dict(lr=0.1, momentum=1.0),
           dict(lr=0.1, momentum=-0.1), dict(lr=0.1, momentum=float("nan")),
           dict(lr=0.1, weight_decay=-1e-4), dict(lr=0.1, weight_decay=float("inf")),
           dict(lr=0.1, nesterov=True), dict(lr=0.1, skip_nonfinite=True)]
    p0, m0 = p.copy(), m.copy()
    for kw in bad:
        with pytest.raises(ValueError):
            comp.apply_sgd_many([p], [h], [m], **kw)
    with pytest.raises(ValueError):
        comp.apply_sgd_many([p], [h], [m], 0, **ok)                      # divisor < 1
    with pytest.raises(ValueError):
        comp.apply_sgd_many([p, p], [h], [m], **ok)                      # counts
    with pytest.raises(ValueError):
        comp.apply_sgd_many([p.astype(np.float64)], [h], [m], **ok)      # f64 parameter
    with pytest.raises(ValueError):
        comp.apply_sgd_many([p], [h], [m.astype(np.float64)], **ok)      # f64 momentum
    with pytest.raises(ValueError):
        comp.apply_sgd_many([p], [h[:-1]], [m], **ok)                    # sizes
    with pytest.raises(ValueError):
        comp.apply_sgd_many([p], [h.view(np.uint16)], [m], **ok)         # not this wire's dtype
    with pytest.raises(ValueError):
        Compression.bf16.apply_sgd_many([p], [h], [m], **ok)
    with pytest.raises(ValueError):
        comp.apply_sgd_many([np.zeros((4, 8), np.float32).T], [h[:32]], [np.zeros(32, np.float32)],
                            **ok)                                        # not contiguous
    assert np.array_equal(_bits(p), _bits(p0)) and np.array_equal(_bits(m), _bits(m0))
    with pytest.raises(ValueError):
        sgd.wire_to_f32(h, "fp8")
    with pytest.raises(ValueError):
        sgd.sgd_step(p, m[:-1], h, "fp16", lr=0.1)


def test_push_pull_iteration_apply_errors_before_anything_is_pushed():
    """The ValueErrors of push_pull_iteration(apply=) need no server: they are
    raised before the first push."""
    from prophet_amd.pushpull import Context, SgdStep, Worker

    class NoTraffic:
        size = 2

        def push(self, *a):
            raise AssertionError("pushed")

        def pull(self, *a):
            raise AssertionError("pulled")

    w = Worker(0, NoTraffic())

    def ctx(name, data, compression):
        c = Context(name, w.declare(name))
        if compression.compresses(data):
            c.compressor, c.staging = compression, compression.wire_like(data)
            c.extra = None
        c.parts, c.initialized = [], True
        w.contexts[name] = c
        return data

    g = ctx("g", np.ones(16, np.float32), Compression.fp16)
    i = ctx("i", np.ones(4, np.int32), Compression.fp16)
    params = {"g": np.zeros(16, np.float32)}
    # well-formed: nothing to push (no partitions), the step runs on the host
    w.push_pull_iteration({"g": g, "i": i}, apply=SgdStep(params, lr=0.5))
    assert w.momentum("g") is not None and w.momentum("i") is None
    w.reset_momentum("g")
    assert not w.momentum("g").any()
    w.reset_momentum("i")
    plain = ctx("plain", np.ones(8, np.float32), Compression.none)
    with pytest.raises(ValueError, match="not compressed"):
        w.push_pull_iteration({"plain": plain}, apply=SgdStep({"plain": plain.copy()}, lr=0.5))
    f64 = ctx("f64", np.ones(8, np.float64), Compression.fp16)
    with pytest.raises(ValueError, match="float32"):
        w.push_pull_iteration({"f64": f64}, apply=SgdStep({"f64": f64.copy()}, lr=0.5))
    with pytest.raises(ValueError, match="no parameter"):
        w.push_pull_iteration({"g": g}, apply=SgdStep({}, lr=0.5))
    with pytest.raises(ValueError, match="differs"):
        w.push_pull_iteration({"g": g}, apply=SgdStep({"g": np.zeros(15, np.float32)}, lr=0.5))
    with pytest.raises(ValueError, match="differs"):
        w.push_pull_iteration({"g": g}, apply=SgdStep({"g": torch.zeros(16)}, lr=0.5))
    with pytest.raises(ValueError, match="clip_norm"):
        w.push_pull_iteration({"g": g}, apply=SgdStep(params, lr=0.5, skip_nonfinite=True))
    with pytest.raises(ValueError):
        w.push_pull_iteration({"g": g}, apply=SgdStep(params, lr=0.5, nesterov=True))


def test_plan_cache_keys_sgd_plans_apart():
    """An SGD plan over the addresses of an error-feedback plan is another
    entry (no library call: the creators are stubbed)."""
    from prophet_amd import compression

    class T:
        def __init__(self, ptr, n):
            self._p, self._n = ptr, n

        def data_ptr(self):
            return self._p

        def numel(self):
            return self._n

    made = []
    real = compression._new_plan, compression._new_sgd_plan

    class P:
        def close(self):
            pass

    compression._new_plan = lambda *a: made.append("cast") or P()
    compression._new_sgd_plan = lambda *a: made.append("sgd") or P()
    try:
        cache = CastPlanCache(4)
        a, b, c = T(4096, 8), T(8192, 8), T(12288, 8)
        ef = cache.get(0, [(a, b, c)], 2)
        s = cache.get_sgd([(a, b, c)], 2)
        assert ef is not s and made == ["cast", "sgd"] and len(cache) == 2
        assert cache.get_sgd([(a, b, c)], 2) is s and cache.get(0, [(a, b, c)], 2) is ef
        assert cache.get_sgd([(a, b, c)], 11) is not s       # another wire
        assert cache.built == 3
        cache.close()
    finally:
        compression._new_plan, compression._new_sgd_plan = real
