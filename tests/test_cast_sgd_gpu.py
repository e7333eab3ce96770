"""The SGD step inside the decompress on the GPU:
byteps_reduce_cast_plan_create_sgd / _apply_sgd (cast_sgd_kernel,
prophet_amd/csrc/bpsr_cast_sgd.h), both wires, at 1, 2 and 4 units a lane and
under both store policies, bit for bit against prophet_amd/sgd.py.

One plan per wire holds every path (tests/cast_shapes.py's shapes with a third
operand): a main segment (head of 3, three or more full tiles, all 65,536
wire patterns in order from an odd start, a partial tile of kBlock + 37 units,
tail of 5); a segment whose wire and parameter never co-align (three element
records); a segment whose momentum does not co-align with its parameter
(element path by cast_cut_ef's rule); a parameter at an odd byte address (the
byte-wise path); segments of 8 and of 1 element; and, for U 2 and 4, the
kMinTiles ballast of 8-element segments in one arena per operand with 16
sentinel bytes between neighbours.  Every operand lies between 0xA5 bytes.

Parameters and momenta come from cast_shapes.wide_table (random magnitudes
over 2^-30 .. 2^20, signed zeros, f32 subnormals, infinities, NaNs) with
values whose ``wd * p`` and ``lr * d`` are subnormal written over a few
places; one case starts from a zero momentum.

Checks, per case: p' and m' equal sgd.py on the host copies (NaN positions as
NaN-ness); with a record they also equal sgd.py's update applied to the bytes
``decompress(scale=record.mult)`` writes into a twin gradient buffer; the
wire bytes and every sentinel byte around all three operands are unchanged; a
second apply from the first one's outputs equals two steps of the definition;
the launch repeated on restored inputs gives the same bits.  The skip, and
every EARGS / EDTYPE case, leave every byte.

The tile size and the store policy come from the library's tuning, which a
process reads once: U 1 runs here (a small plan, write-through), U 2
(non-temporal) and U 4 (write-through) in child processes, this file run as a
script with BPSR_COPY_VPT and BPSR_WT_MAX_MIB, as tests/test_cast_clip_gpu.py
does."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import cast_shapes as cs  # noqa: E402
from prophet_amd import reducer, sgd  # noqa: E402
from prophet_amd.dtypes import DType  # noqa: E402
from prophet_amd.reducer import GpuReducer, SrKey  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

WIRE_ID = {"fp16": int(DType.FLOAT16), "bf16": int(DType.BFLOAT16)}
F32_ID = int(DType.FLOAT32)
SENT = cs.SENTINEL
CANON = np.uint32(0x7fc00000)

# (divisor, record, (momentum, weight_decay, nesterov), momentum starts at zero)
CASES = [
    (1, False, (0.0, 0.0, False), False),
    (8, False, (0.9, 0.0, False), False),
    (8, True, (0.9, 1e-4, False), False),
    (1, True, (0.9, 1e-4, True), False),
    (8, False, (0.9, 1e-4, True), True),
]
LR = 0.1
# child processes: name -> (BPSR_COPY_VPT, BPSR_WT_MAX_MIB): U 2 with
# non-temporal stores, U 4 with write-through stores
CHILDREN = {"u2nt": (2, 0), "u4wt": (4, 1024)}


@pytest.fixture(scope="module")
def red():
    assert torch.cuda.is_available()
    return GpuReducer(device=0)


class Group:
    """Segments of n elements each: byte offsets of every segment's operands
    in the images of the parameter (W), wire (H) and momentum (M) buffers."""

    def __init__(self, n, ow, oh, om):
        self.n = n
        self.off = {"W": np.asarray(ow, np.int64), "H": np.asarray(oh, np.int64),
                    "M": np.asarray(om, np.int64)}

        self._idx = {}

    def idx(self, which):
        """The byte positions of every element of the group's segments."""
        if which not in self._idx:
            es = 2 if which == "H" else 4
            self._idx[which] = (self.off[which][:, None] +
                                np.arange(self.n * es)[None, :]).reshape(-1)
        return self._idx[which]


class Layout:
    """The plan's segments laid out in one image per operand."""

    def __init__(self, u):
        self.u = u
        self.groups = []
        self.pos = {"W": 256, "H": 256, "M": 256}
        k = cs.HEAD
        # main: wire and parameter co-align after k elements, the momentum with the parameter
        self.add(cs.main_elems(u), (16 - 4 * (k % 4)) % 16, (16 - 2 * k) % 16,
                 (16 - 4 * (k % 4)) % 16)
        self.add(cs.NEVER, 0, 2, 0)          # wire and parameter never co-align
        self.add(cs.TILE1 + 77, 0, 0, 4)     # the momentum does not co-align with the parameter
        self.add(100, 1, 0, 0)               # a parameter at an odd byte address
        self.add(8, 0, 0, 0)
        self.add(1, 0, 0, 0)
        if u > 1:
            self.ballast()
        self.size = {w: self.pos[w] + 256 for w in self.pos}

    def add(self, n, aw, ah, am):
        offs = {}
        for w, add, es in (("W", aw, 4), ("H", ah, 2), ("M", am, 4)):
            p = -(-self.pos[w] // 256) * 256 + add
            offs[w] = [p]
            self.pos[w] = p + n * es + 256
        self.groups.append(Group(n, offs["W"], offs["H"], offs["M"]))

    def ballast(self):
        offs = {}
        for w, es in (("W", 4), ("H", 2), ("M", 4)):
            base = -(-self.pos[w] // 256) * 256
            stride = 8 * es + 16
            offs[w] = base + stride * np.arange(cs.NSEG)
            self.pos[w] = base + stride * cs.NSEG + 256
        self.groups.append(Group(8, offs["W"], offs["H"], offs["M"]))

    def tiles(self, u):
        """Vector tiles of the plan cut for u (the table builder's rule)."""
        t = 0
        for g, nseg in ((g, len(g.off["W"])) for g in self.groups):
            w, h, m = (int(g.off[x][0]) for x in "WHM")
            if w % 4 or m % 4 or (w - m) % 16:
                continue
            hh, hw = ((16 - h % 16) % 16) // 2, ((16 - w % 16) % 16) // 4
            if hh % 4 != hw or hh >= g.n:
                continue
            units = (g.n - hh) // 8
            t += nseg * -(-units // (cs.K_BLOCK * u))
        return t


def _images(lay, wire, zero_m):
    """The three host images: sentinels, the segments' values written in."""
    img = {w: np.full(lay.size[w], SENT, np.uint8) for w in "WHM"}
    table = cs.wide_table(4)
    at = 0
    for gi, g in enumerate(lay.groups):
        nseg = len(g.off["W"])
        tot = nseg * g.n
        h = cs.patterns16(tot, (0x3c01 + 74 * gi) & 0xffff)
        p = np.take(table, (np.arange(tot) + 997 * gi + 13) % cs.PERIOD).copy()
        m = np.take(table, (np.arange(tot) + 31337 + 499 * gi) % cs.PERIOD).copy()
        if g.n > 64:
            # wd * p subnormal (1e-4 * 2^-115), and lr * d subnormal: a zero
            # gradient on the wire over a momentum of 2^-124
            p[5::97] = np.float32(2.0 ** -115)
            h[7::101] = 0x8000 if gi % 2 else 0
            m[7::101] = np.float32(-(2.0 ** -124))
        if zero_m:
            m[:] = 0
        img["H"][g.idx("H")] = h.view(np.uint8)
        img["W"][g.idx("W")] = p.view(np.uint8)
        img["M"][g.idx("M")] = m.view(np.uint8)
        at += tot
    return img


def _gather(img, g, which):
    b = img[which][g.idx(which)]
    return b.view(np.uint16 if which == "H" else np.float32)


def _canon(img, lay, which):
    """The image with every NaN of its segments as one pattern."""
    out = img.copy()
    for g in lay.groups:
        v = out[g.idx(which)].view(np.uint32)
        v[np.isnan(v.view(np.float32))] = CANON
        out[g.idx(which)] = v.view(np.uint8)
    return out


class Device:
    """The images on the device, each from a 256-byte aligned address."""

    def __init__(self, lay, img):
        self.raw, self.view, self.base = {}, {}, {}
        for w in img:
            raw = torch.empty(lay.size[w] + 256, dtype=torch.uint8, device="cuda")
            shift = (-raw.data_ptr()) % 256
            self.raw[w], self.view[w] = raw, raw[shift:shift + lay.size[w]]
            self.base[w] = raw.data_ptr() + shift
        self.load(img)

    def load(self, img):
        for w in img:
            self.view[w].copy_(torch.from_numpy(img[w]))

    def read(self, which):
        return self.view[which].cpu().numpy()


def _descs(lay, dev, wide="W"):
    out = []
    for g in lay.groups:
        for s in range(len(g.off["W"])):
            out.append((dev.base[wide] + int(g.off["W"][s]), dev.base["H"] + int(g.off["H"][s]),
                        g.n, dev.base["M"] + int(g.off["M"][s])))
    return out


def _step(lay, img, wire, divisor, hyper, mult):
    """The definition over every segment: the expected images."""
    mu, wd, nesterov = hyper
    out = {w: img[w].copy() for w in img}
    for g in lay.groups:
        pn, mn = sgd.sgd_step(_gather(img, g, "W"), _gather(img, g, "M"), _gather(img, g, "H"),
                              wire, divisor, lr=LR, momentum=mu, weight_decay=wd,
                              nesterov=nesterov, mult=mult)
        out["W"][g.idx("W")] = pn.view(np.uint8)
        out["M"][g.idx("M")] = mn.view(np.uint8)
    return out


def _expect(lay, dev, want, what):
    for w in "WM":
        got = dev.read(w)
        a, b = _canon(got, lay, w), _canon(want[w], lay, w)
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b)
            raise AssertionError(f"{what}: buffer {w} differs at {bad.size} bytes, first "
                                 f"{bad[:8].tolist()} of {a.size}")
    assert np.array_equal(dev.read("H"), want["H"]), f"{what}: the wire bytes changed"


def _record(red, inv, nonfinite=0.0):
    """A clip record made on the device: norm 5 * inv against max_norm
    0.0123; its mult read back."""
    rows = torch.tensor([[9.0, nonfinite], [16.0, 0.0]], dtype=torch.float64, device="cuda")
    inv_t = torch.tensor([inv], dtype=torch.float32, device="cuda")
    rec = red.clip_record(rows, 0.0123, 1e-6, inv_t)
    mult = np.float32(rec.mult.cpu().numpy())
    assert float(rec.nonfinite) == nonfinite and 0 < float(mult) < inv
    return rec, mult


def _run_wire(red, u, wire):
    cur = torch.cuda.current_stream()
    lay = Layout(u)
    if u > 1:
        assert lay.tiles(u) >= cs.K_MIN_TILES, "the plan keeps the tuned tile size"
    else:
        assert lay.tiles(2) < cs.K_MIN_TILES, "a small plan is cut for one unit a lane"
    img0 = _images(lay, wire, False)
    dev = Device(lay, img0)
    plan = red.sgd_plan(_descs(lay, dev), WIRE_ID[wire])
    # the twin gradient buffer: the plain plan over (G, H) at the parameter's offsets
    grad = torch.full((lay.size["W"] + 256,), SENT, dtype=torch.uint8, device="cuda")
    gshift = (-grad.data_ptr()) % 256
    gbase = grad.data_ptr() + gshift
    twin_descs = [(gbase + (d[0] - dev.base["W"]), d[1], d[2]) for d in _descs(lay, dev)]
    twin = red.cast_plan(twin_descs, F32_ID, WIRE_ID[wire])
    rec, mult = _record(red, 2.0 ** -7)
    for divisor, with_rec, hyper, zero_m in CASES:
        what = f"u={u} {wire} divisor={divisor} record={with_rec} {hyper} zero_m={zero_m}"
        img = _images(lay, wire, zero_m)
        kw = dict(lr=LR, momentum=hyper[0], weight_decay=hyper[1], nesterov=hyper[2],
                  record=rec if with_rec else None, stream=cur)
        m = mult if with_rec else None
        one = _step(lay, img, wire, divisor, hyper, m)
        dev.load(img)
        plan.apply(divisor, **kw)
        _expect(lay, dev, one, what)
        first = {w: dev.read(w) for w in "WM"}
        # a second apply continues from the first one's outputs
        two = _step(lay, {"W": first["W"], "M": first["M"], "H": img["H"]}, wire, divisor,
                    hyper, m)
        plan.apply(divisor, **kw)
        _expect(lay, dev, two, what + " second step")
        # the same launch on restored inputs: the same bits, NaN payloads included
        dev.load(img)
        plan.apply(divisor, **kw)
        for w in "WM":
            assert np.array_equal(dev.read(w), first[w]), what + " repeated"
        if with_rec:
            # "apply" agrees with "scaled decompress, then the step"
            twin.decompress(divisor, stream=cur, scale=rec.mult)
            gimg = grad[gshift:gshift + lay.size["W"]].cpu().numpy()
            want = {w: img[w].copy() for w in img}
            for g in lay.groups:
                gv = gimg[g.idx("W")].view(np.float32)
                pn, mn = sgd.sgd_update(_gather(img, g, "W"), _gather(img, g, "M"), gv, lr=LR,
                                        momentum=hyper[0], weight_decay=hyper[1],
                                        nesterov=hyper[2])
                want["W"][g.idx("W")] = pn.view(np.uint8)
                want["M"][g.idx("M")] = mn.view(np.uint8)
            _expect(lay, dev, want, what + " against the scaled decompress")
    # ---- skip
    img = img0
    found, fmult = _record(red, 2.0 ** -7, nonfinite=1.0)
    hyper = (0.9, 1e-4, True)
    kw = dict(lr=LR, momentum=0.9, weight_decay=1e-4, nesterov=True, stream=cur)
    dev.load(img)
    plan.apply(8, record=found, skip_nonfinite=True, **kw)
    for w in "WHM":
        assert np.array_equal(dev.read(w), img[w]), f"u={u} {wire}: a skipped step wrote {w}"
    plan.apply(8, record=found, skip_nonfinite=False, **kw)
    _expect(lay, dev, _step(lay, img, wire, 8, hyper, fmult), f"u={u} {wire} no skip asked")
    dev.load(img)
    plan.apply(8, record=rec, skip_nonfinite=True, **kw)
    _expect(lay, dev, _step(lay, img, wire, 8, hyper, mult), f"u={u} {wire} nothing to skip")
    torch.cuda.synchronize()
    twin.close()
    plan.close()


@pytest.mark.parametrize("wire", ["fp16", "bf16"])
def test_apply_sgd_one_unit_tiles(red, wire):
    _run_wire(red, 1, wire)


@pytest.mark.parametrize("child", sorted(CHILDREN))
def test_apply_sgd_larger_tiles_in_a_child_process(child):
    vpt, wt = CHILDREN[child]
    env = dict(os.environ, BPSR_COPY_VPT=str(vpt), BPSR_WT_MAX_MIB=str(wt))
    r = subprocess.run([sys.executable, os.path.abspath(__file__), child], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert f"{child} cases passed" in r.stdout


# ------------------------------------------------------------------- errors --
def _small(red, wire="fp16", n=cs.TILE1 + 9):
    g = torch.Generator(device="cuda").manual_seed(3)
    p = torch.randn(n, generator=g, device="cuda")
    m = torch.randn(n, generator=g, device="cuda")
    h = torch.randn(n, generator=g, device="cuda").to(
        torch.float16 if wire == "fp16" else torch.bfloat16)
    return p, h, m


def test_bad_arguments_raise_before_any_launch(red):
    cur = torch.cuda.current_stream()
    lib, stream = red.lib, int(cur.cuda_stream)
    p, h, m = _small(red)
    n = p.numel()
    before = [x.clone() for x in (p, h, m)]
    plan = red.sgd_plan([(p, h, n, m)], WIRE_ID["fp16"])
    rec, _ = _record(red, 0.5)
    ok = dict(lr=0.1, momentum=0.9, weight_decay=1e-4)

    def eargs(call, *a, **kw):
        with pytest.raises(reducer.ReduceError) as e:
            call(*a, **kw)
        assert e.value.code == reducer.EARGS
        return str(e.value)

    inf, nan = float("inf"), float("nan")
    eargs(plan.apply, 0, **ok)                                       # divisor < 1
    for lr in (inf, -inf, nan):
        eargs(plan.apply, 1, lr=lr)
    for mu in (1.0, -0.5, 1.5, nan):
        eargs(plan.apply, 1, lr=0.1, momentum=mu)
    for wd in (-1e-4, inf, nan):
        eargs(plan.apply, 1, lr=0.1, weight_decay=wd)
    eargs(plan.apply, 1, lr=0.1, nesterov=True)                      # momentum == 0
    eargs(plan.apply, 1, skip_nonfinite=True, **ok)                  # no record
    eargs(plan.apply, 1, record=rec.tensor.data_ptr() + 4, **ok)     # not 8-byte aligned
    eargs(plan.apply, 1, record=p.data_ptr(), **ok)                  # inside the parameter
    assert (4 * n - 4) % 8 == 0
    eargs(plan.apply, 1, record=m.data_ptr() + 4 * n - 4, **ok)      # the momentum's last 4 bytes
    eargs(plan.apply, 1, record=h.data_ptr() - 24, **ok)             # 8 bytes into the wire
    f = lib.byteps_reduce_cast_plan_apply_sgd
    hy = reducer.SgdHyper(0.1, 0.9, 0.0, 0)
    import ctypes
    assert f(None, 1, ctypes.byref(hy), None, 0, stream) == reducer.EARGS      # null plan
    assert f(plan.handle, 1, None, None, 0, stream) == reducer.EARGS           # null h
    # every other plan call is refused on an SGD plan and names _apply_sgd
    stats = torch.zeros(2, dtype=torch.float64, device="cuda")
    one = torch.ones(1, device="cuda")
    for rc in (lib.byteps_reduce_cast_plan_compress(plan.handle, stream),
               lib.byteps_reduce_cast_plan_compress_sr(plan.handle, 3, stream),
               lib.byteps_reduce_cast_plan_decompress(plan.handle, 1, stream),
               lib.byteps_reduce_cast_plan_decompress_stats(plan.handle, 1, stats.data_ptr(),
                                                            stream),
               lib.byteps_reduce_cast_plan_measure(plan.handle, 1, stats.data_ptr(), stream),
               lib.byteps_reduce_cast_plan_decompress_scaled(plan.handle, 1, one.data_ptr(),
                                                             stream)):
        assert rc == reducer.EARGS
        assert b"apply_sgd" in lib.byteps_reduce_last_error()
    # apply_sgd is refused on plain, error-feedback and stochastic-rounding plans
    g = torch.zeros(n, device="cuda")
    r = torch.zeros(n, device="cuda")
    for segs in ([(g, h, n)], [(g, h, n, r)], [(g, h, n, SrKey(5))]):
        other = red.cast_plan(segs, F32_ID, WIRE_ID["fp16"])
        assert f(other.handle, 1, ctypes.byref(hy), None, 0, stream) == reducer.EARGS
        assert b"create_sgd" in lib.byteps_reduce_last_error()
        other.close()
    # create: the wire dtype, null pointers, overlapping ranges
    def create(segs, wire):
        with pytest.raises(reducer.ReduceError) as e:
            red.sgd_plan(segs, wire)
        return e.value.code

    assert create([(p, h, n, m)], F32_ID) == reducer.EDTYPE
    assert create([(p, h, n, m)], int(DType.FLOAT64)) == reducer.EDTYPE
    assert create([(0, h, n, m)], WIRE_ID["fp16"]) == reducer.EARGS
    assert create([(p, 0, n, m)], WIRE_ID["fp16"]) == reducer.EARGS
    assert create([(p, h, n, 0)], WIRE_ID["fp16"]) == reducer.EARGS
    assert create([(p, h, n, p)], WIRE_ID["fp16"]) == reducer.EARGS            # m is p
    assert create([(p, h, n, m.data_ptr() - 0), (g, h.data_ptr() + 2 * n - 2, 1, r)],
                  WIRE_ID["fp16"]) == reducer.EARGS                            # wires overlap
    assert create([(p, h, 8, m), (g, h[8:], 8, p.data_ptr() + 16)],
                  WIRE_ID["fp16"]) == reducer.EARGS       # a momentum inside another's parameter
    with pytest.raises(ValueError):
        red.sgd_plan([(p, h, n + 1, m)], WIRE_ID["fp16"])                      # bounds, in Python
    with pytest.raises(ValueError):
        red.sgd_plan([(p, h, n)], WIRE_ID["fp16"])
    with pytest.raises(ValueError):
        plan.apply(1, record=torch.zeros(32, dtype=torch.uint8, device="cuda"), **ok)
    torch.cuda.synchronize()
    for x, b in zip((p, h, m), before):
        assert torch.equal(x.view(torch.int16), b.view(torch.int16))           # nothing ran
    # plans without records: nothing to launch
    red.sgd_plan([], WIRE_ID["bf16"]).apply(1, **ok)
    hollow = red.sgd_plan([(0, 0, 0, 0), (0, 0, 0, 0)], WIRE_ID["bf16"])
    hollow.apply(3, record=rec, skip_nonfinite=True, **ok)
    hollow.close()
    plan.close()


# -------------------------------------------------------------- compressors --
@pytest.mark.parametrize("wire", ["fp16", "bf16"])
def test_compressor_apply_on_the_device(wire):
    """apply_sgd_many over cached SGD plans, and the one-tensor form."""
    from prophet_amd.compression import CastPlanCache, Compression
    comp = getattr(Compression, wire)
    sizes = [300, cs.TILE1 + 9, 1, 2 * cs.TILE1]
    trio = [_small(None, wire, n) for n in sizes]
    ps, hs, ms = ([t[i] for t in trio] for i in range(3))
    red = GpuReducer(device=0)
    rec, mult = _record(red, 2.0 ** -3)
    kw = dict(lr=0.05, momentum=0.9, weight_decay=1e-4, nesterov=True)
    cache = CastPlanCache(4)
    for step in range(2):
        want = [sgd.sgd_step(p.cpu().numpy(), m.cpu().numpy(),
                             h.cpu().view(torch.int16).numpy().view(np.uint16), wire, 8,
                             mult=mult, **kw) for p, h, m in zip(ps, hs, ms)]
        out = comp.apply_sgd_many(ps, hs, ms, 8, record=rec, skip_nonfinite=True, plans=cache,
                                  **kw)
        assert out is ps and cache.built == 1, "the second round reuses the plan"
        for p, m, (pn, mn) in zip(ps, ms, want):
            assert np.array_equal(p.cpu().numpy().view(np.uint32), pn.view(np.uint32))
            assert np.array_equal(m.cpu().numpy().view(np.uint32), mn.view(np.uint32))
    # an error-feedback plan over the same three addresses is another plan
    cache.get(F32_ID, [(ps[0], hs[0], ms[0])], WIRE_ID[wire])
    assert cache.built == 2 and len(cache) == 2
    cache.close()
    p, h, m = _small(None, wire, 77)
    pn, mn = sgd.sgd_step(p.cpu().numpy(), m.cpu().numpy(),
                          h.cpu().view(torch.int16).numpy().view(np.uint16), wire, 1, lr=0.5)
    assert comp.apply_sgd_into(p, h, m, lr=0.5) is p
    assert np.array_equal(p.cpu().numpy().view(np.uint32), pn.view(np.uint32))
    assert np.array_equal(m.cpu().numpy().view(np.uint32), mn.view(np.uint32))
    with pytest.raises(ValueError):
        comp.apply_sgd_many([p], [h], [m.cpu()], lr=0.5)                 # two places
    with pytest.raises(ValueError):
        comp.apply_sgd_many([p], [h.float()], [m], lr=0.5)               # not the wire dtype
    with pytest.raises(ValueError):
        from prophet_amd.compression import ClipValues
        comp.apply_sgd_many([p], [h], [m], lr=0.5,
                            record=ClipValues(1.0, 0.0, 1.0, np.float32(1), np.float32(1)))


if __name__ == "__main__":
    _child = sys.argv[1]
    _u = CHILDREN[_child][0]
    _red = GpuReducer(device=0)
    for _wire in ("fp16", "bf16"):
        _run_wire(_red, _u, _wire)
    print(f"{_child} cases passed")
