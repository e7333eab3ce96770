"""The cast kernels (cast_kernel, cast_plan_kernel and its STATS variant;
prophet_amd/csrc/bpsr_cast_single.h, bpsr_cast_plan.h) at 1, 2 and 4 units a
lane, under both store policies, for every wire and wide type, bit for bit
against the host definitions.

Matrix: wire {fp16, bf16} x wide {f32, f64, the other 2-byte float} x
{compress, decompress with divisors 1, 3 and 8}, each through the one-tensor
call, the plan and the plan with ``stats=``, each at U {1, 2, 4} x {write-
through, non-temporal}; and for f32 the error-feedback compress (wire and
residual) and the stochastic-rounding compress through the plan at U 2 and 4.

The tile size and the policy come from the library's tuning, which a process
reads once, so the matrix runs in four processes (cast_shapes.ENVS): this one
(U 1 and 2, write-through) and three children, this file run as a script, one
after the other — BPSR_COPY_VPT=4 BPSR_WT_MAX_MIB=1024 (U 4, write-through),
BPSR_WT_MAX_MIB=0 (U 1 and 2, non-temporal) and both (U 4, non-temporal).
Nothing here can see U or the policy: tests/test_cast_shapes.py asserts on the
CPU that every shape used here gets the U and the policy named, and that the
tables hold the records named.

Shapes (tests/cast_shapes.py): a plan keeps the tuned U while it has
kMinTiles tiles, and a segment of 8 elements is one tile at any U, so the
plans are a main segment (head of 3, full tiles, a partial tile of
kBlock + 37 units, tail of 5; 65,537 elements and more), a segment that never
co-aligns (three element records) and a ballast of kMinTiles 8-element
segments in one arena a side — guarded-tile records of one unit.  The
one-tensor calls need kMinTiles - 1 full tiles and the partial one: 8 Mi
elements at U 2, 16 Mi at U 4.  Their source and expected output are computed
on the host for one period of 65,537 elements and expanded on the device.

Data: 2-byte sources are all 65,536 patterns in order from an odd start;
f32 / f64 sources are cast_shapes.wide_table (ties, overflow thresholds,
subnormal results, f32 subnormals, signed zeros, infinities, NaN payloads, f64
values that round twice, random magnitudes) with edge values at the head, at
lanes 0 and 255 of the first and last j of every full tile, in the partial
tile and in the tail.

Expected values, the definitions the suite already pins: torch's CPU casts
(f64 through f32); ``div_`` on the CPU wire tensor, then the widening cast;
tests/test_cast_nt_gpu.py's host_ef; prophet_amd/sr.py.  Raw bytes are
compared; where the expected value is a NaN, a NaN is required.  Every
destination lies between 0xA5 bytes, which must stay (the gaps of the ballast
arenas too); no source may change.

Statistics: the non-finite count equals tests/test_cast_stats_gpu.py's
definition applied to the bytes written; the sum of squares equals it bit for
bit on small integers times powers of two, and within that file's
``nelem * 2**-52 * ref`` any-order bound on the all-patterns run; the bytes of
a decompress with statistics are the plain plan's.

Two one-line mutants of cast_tile_full, each right at U 1 — the 2-byte wide
compress branch loading every x[j] from j = 0, and the f64 decompress re-deal
reading h[0] for every j — pass every other test of the suite and fail this
file at U 2 and 4."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

import cast_shapes as cs  # noqa: E402
from prophet_amd import sr  # noqa: E402
from prophet_amd.dtypes import from_torch  # noqa: E402
from prophet_amd.reducer import GpuReducer, SrKey  # noqa: E402
from test_cast_nt_gpu import host_ef  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(240)]

F16, BF16, F32, F64 = torch.float16, torch.bfloat16, torch.float32, torch.float64
WIRE = {"fp16": F16, "bf16": BF16}
PAIRS = [(w, x) for w in cs.WIRES for x in cs.WIDE_ES]
DIVISORS = (1, 3, 8)
KEY, STEP = 0x1234abcd, 5
NAN = float("nan")
_INT = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _wide(wire, name):
    return {"f32": F32, "f64": F64, "x16": BF16 if wire == "fp16" else F16}[name]


def _tensor(a, dt):
    """A numpy array of bit patterns or values as a CPU tensor of dtype dt."""
    a = np.array(a)                                   # a copy: shared tables are read-only
    return torch.from_numpy(a.view({1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.itemsize])
                            ).view(dt)


# ------------------------------------------------------------ definitions --
def ref_compress(x, wire):
    """tests/test_compress_gpu.py, test_compress_bf16_gpu.py: torch's CPU
    cast, f64 through f32."""
    return (x.to(F32) if x.dtype == F64 else x).to(wire)


def ref_decompress(h, d, wide):
    """The divide on the wire tensor, rounded to the wire format, then the
    widening cast (tests/test_cast_nt_gpu.py)."""
    return (h.clone().div_(d) if d > 1 else h).to(wide)


def _definition(x):
    """tests/test_cast_stats_gpu.py's: the f64 sum of the squares of the
    finite values and the count of the others."""
    x = x.to(F64).numpy().reshape(-1)
    fin = np.isfinite(x)
    return float(np.square(x[fin]).sum()), int(np.count_nonzero(~fin))


def _same(got, want):
    """Bit for bit, but a NaN where a NaN is expected."""
    ib = _INT[want.element_size()]
    return bool(((got.view(ib) == want.view(ib)) | (torch.isnan(want) & torch.isnan(got))).all())


# ----------------------------------------------------------------- memory --
class Arena:
    """Segments of `counts` elements of `dt` at byte offsets `offs` of `size`
    bytes of device memory from a 256-byte aligned address, 0xA5 elsewhere."""

    def __init__(self, offs, counts, dt, size):
        self.es = es = torch.empty((), dtype=dt).element_size()
        size = -(-size // 16) * 16
        self.raw = torch.full((size + 256,), cs.SENTINEL, dtype=torch.uint8, device="cuda")
        base = (-self.raw.data_ptr()) % 256
        self.bytes = self.raw[base:base + size]
        self.typed = self.bytes.view(dt)
        self.offs, self.counts = list(offs), list(counts)
        self.ptrs = [self.bytes.data_ptr() + o for o in offs]
        self.one = len(offs) == 1
        assert all(o % es == 0 and 0 <= o and o + n * es <= size for o, n in zip(offs, counts))
        if not self.one:                                 # small: index and mask from the host
            self.idx = torch.from_numpy(np.concatenate(
                [o // es + np.arange(n, dtype=np.int64) for o, n in zip(offs, counts)])).cuda()
            outside = np.ones(size, bool)
            for o, n in zip(offs, counts):
                assert o % es == 0 and o + n * es <= size and outside[o:o + n * es].all()
                outside[o:o + n * es] = False
            self.outside = torch.from_numpy(outside).cuda()

    def seg(self, i=0):
        lo = self.offs[i] // self.es
        return self.typed[lo:lo + self.counts[i]]

    def put(self, values):
        """The segments' values, one after the other (a device or host tensor)."""
        if self.one:
            self.seg().copy_(values)
        else:
            self.typed[self.idx] = values.cuda()

    def get(self):
        return self.seg() if self.one else self.typed[self.idx]

    def reset(self):
        self.raw.fill_(cs.SENTINEL)

    def intact(self):
        """Every byte outside the segments is still 0xA5."""
        if self.one:
            lo, hi = self.offs[0], self.offs[0] + self.counts[0] * self.es
            return bool((self.raw[:self.raw.numel() - self.bytes.numel()] == cs.SENTINEL).all()) \
                and bool((self.bytes[:lo] == cs.SENTINEL).all()) \
                and bool((self.bytes[hi:] == cs.SENTINEL).all())
        return bool((self.bytes[self.outside] == cs.SENTINEL).all())


def _arenas(segs, wire, wide, resid=False):
    es = torch.empty((), dtype=wide).element_size()
    woffs, hoffs, wsize, hsize = cs.layout(segs, es)
    counts = [n for _, n, _ in segs]
    out = [Arena(woffs, counts, wide, wsize), Arena(hoffs, counts, wire, hsize)]
    if resid:
        out.append(Arena(woffs, counts, F32, wsize))
    return out


# ------------------------------------------------------ the one-tensor call --
_PER = {}


def _per(n):
    """arange(n) % PERIOD on the device; the latest one is kept."""
    if n not in _PER:
        _PER.clear()
        _PER[n] = torch.arange(n, device="cuda") % cs.PERIOD
    return _PER[n]


def _expand(period, n, edge=None):
    """One period of host values as n device values, then ``edge``:
    (positions, which, values) written over them."""
    x = period.cuda()[_per(n)]
    if edge is not None:
        pos, which, vals = edge
        x[torch.from_numpy(pos).cuda()] = vals.cuda()[torch.from_numpy(which).cuda()]
    return x


def run_single(red, wire_name, wide_name, u):
    wire, wide = WIRE[wire_name], _wide(wire_name, wide_name)
    wd, hd = from_torch(wide), from_torch(wire)
    es = cs.WIDE_ES[wide_name]
    segs = cs.segments(u, "single")
    n = segs[0][1]
    W, H = _arenas(segs, wire, wide)
    what = (wire_name, wide_name, u, "single")
    # compress
    if es == 2:
        period, edge, wedge = _tensor(cs.patterns16(cs.PERIOD), wide), None, None
    else:
        period = _tensor(cs.wide_table(es), wide)
        pos, which = cs.edge_index(cs.main_segment(u, n=n), es)
        ev = _tensor(cs.edge_values(es), wide)
        edge, wedge = (pos, which, ev), (pos, which, ref_compress(ev, wire))
    W.put(_expand(period, n, edge))
    before = W.raw.clone()
    red.compress(H.seg(), W.seg(), n, wd, hd)
    assert _same(H.seg(), _expand(ref_compress(period, wire), n, wedge)), what
    assert H.intact() and torch.equal(W.raw, before), what
    del before
    # decompress: every wire pattern
    period = _tensor(cs.patterns16(cs.PERIOD), wire)
    H.reset()
    H.put(_expand(period, n))
    before = H.raw.clone()
    for d in DIVISORS:
        W.reset()
        red.decompress(W.seg(), H.seg(), n, wd, hd, d)
        assert _same(W.seg(), _expand(ref_decompress(period, d, wide), n)), what + (d,)
        assert W.intact() and torch.equal(H.raw, before), what + (d,)


# ---------------------------------------------------------------- the plan --
def _exact_values(n, wire, seed):
    """tests/test_cast_stats_gpu.py's _exact: small integers times powers of
    two, whose squares add up exactly in f64 in any order, also after a divide
    by 8 and in either 2-byte wide type."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-8, 9, n).astype(np.float32) * np.exp2(rng.integers(-2, 4, n)).astype(np.float32)
    return torch.from_numpy(v).to(wire)


def _check_stats(st, got, segs, exact, what):
    """Every row of `st` against the definition applied to `got`, the values
    written, segment after segment (the ballast's rows in one numpy call)."""
    rows = st.cpu().view(-1, 2).numpy()
    assert not np.isnan(rows).any(), what
    counts = [n for _, n, _ in segs]
    big = sum(1 for name, _, _ in segs if name != "ballast")
    ref, at = [], 0
    for n in counts[:big]:
        ref.append(_definition(got[at:at + n]))
        at += n
    if big < len(segs):
        x = got[at:].to(F64).numpy().reshape(-1, 8)
        fin = np.isfinite(x)
        ref += list(zip(np.where(fin, np.square(np.where(fin, x, 0.0)), 0.0).sum(axis=1).tolist(),
                        np.count_nonzero(~fin, axis=1).tolist()))
    assert len(ref) == len(rows) == len(segs)
    for i in (0, 1, len(segs) - 1):
        print(f"{what} seg {i} n={counts[i]}: sumsq {float(rows[i, 0])!r} ref {ref[i][0]!r} "
              f"nonfinite {float(rows[i, 1])} ref {ref[i][1]}")
    ss, nf = np.array([r[0] for r in ref]), np.array([float(r[1]) for r in ref])
    bad = rows[:, 1] != nf
    assert not bad.any(), what + (np.flatnonzero(bad)[:5].tolist(),)
    if exact:
        bad = rows[:, 0] != ss
    else:
        bad = ~(np.abs(rows[:, 0] - ss) <= np.array(counts) * 2.0 ** -52 * ss)
    assert not bad.any(), what + (np.flatnonzero(bad)[:5].tolist(),)


def run_plan(red, wire_name, wide_name, u):
    cur = torch.cuda.current_stream()                 # raw pointers name no device
    wire, wide = WIRE[wire_name], _wide(wire_name, wide_name)
    es = cs.WIDE_ES[wide_name]
    segs = cs.segments(u)
    counts = [n for _, n, _ in segs]
    W, H = _arenas(segs, wire, wide)
    plan = red.cast_plan(list(zip(W.ptrs, H.ptrs, counts)), from_torch(wide), from_torch(wire))
    what = (wire_name, wide_name, u, "plan")
    # compress
    src = _tensor(cs.plan_values(es, segs, u), wide)
    W.put(src)
    before = W.raw.clone()
    plan.compress(stream=cur)
    assert _same(H.get(), ref_compress(src, wire).cuda()), what
    assert H.intact() and torch.equal(W.raw, before), what
    # decompress, plain and with statistics: every wire pattern
    src = _tensor(cs.plan_values(2, segs, u), wire)
    H.reset()
    H.put(src)
    before = H.raw.clone()
    for d in DIVISORS:
        W.reset()
        plan.decompress(d, stream=cur)
        assert _same(W.get(), ref_decompress(src, d, wide).cuda()), what + (d,)
        assert W.intact() and torch.equal(H.raw, before), what + (d,)
        plain = W.raw.clone()
        W.reset()
        st = torch.full((2 * len(segs),), NAN, dtype=F64, device="cuda")
        plan.decompress(d, stream=cur, stats=st)
        assert torch.equal(W.raw, plain) and torch.equal(H.raw, before), what + (d, "stats")
        _check_stats(st, W.get().cpu(), segs, False, what + (d,))
    # statistics bit for bit: values whose squares add up exactly
    src = _exact_values(sum(counts), wire, 100 + u)
    H.put(src)
    W.reset()
    st = torch.full((2 * len(segs),), NAN, dtype=F64, device="cuda")
    plan.decompress(8, stream=cur, stats=st)
    assert _same(W.get(), ref_decompress(src, 8, wide).cuda()) and W.intact(), what + ("exact",)
    _check_stats(st, W.get().cpu(), segs, True, what + ("exact",))
    plan.close()


def _sr_bits(segs):
    """sr.sr_bits of every segment under key KEY + its index, one after the
    other; the ballast's 8-element segments (two Philox counters each) in one
    call."""
    parts, small = [], []
    for i, (name, n, _) in enumerate(segs):
        if name == "ballast":
            small.append(KEY + i)
        else:
            assert not small
            parts.append(sr.sr_bits(n, KEY + i, STEP))
    if small:
        x0, x1 = sr.philox2x32(np.arange(2)[None, :], STEP, np.array(small)[:, None])
        lo, sh = np.uint32(0xffff), np.uint32(16)
        parts.append(np.stack([x0 & lo, x0 >> sh, x1 & lo, x1 >> sh], axis=2).reshape(-1))
        assert np.array_equal(parts[-1][-8:], sr.sr_bits(8, small[-1], STEP))
    return np.concatenate(parts)


def run_ef_sr(red, wire_name, u):
    """The two f32-only compresses through the ballast plan."""
    cur = torch.cuda.current_stream()
    wire = WIRE[wire_name]
    segs = cs.segments(u)
    counts = [n for _, n, _ in segs]
    W, H, R = _arenas(segs, wire, F32, resid=True)
    g = _tensor(cs.plan_values(4, segs, u), F32)
    rng = np.random.default_rng(11)
    sign = torch.from_numpy(rng.choice(np.float32([-1.0, 1.0]), g.numel()))
    r = torch.where(torch.isfinite(g), g * 2.0 ** -10 * sign, torch.zeros_like(g))
    W.put(g)
    before = W.raw.clone()
    what = (wire_name, u)
    # error feedback: wire and residual
    R.put(r)
    plan = red.cast_plan(list(zip(W.ptrs, H.ptrs, counts, R.ptrs)), from_torch(F32),
                         from_torch(wire))
    plan.compress(stream=cur)
    want_w, want_r = host_ef(g, r, wire)
    assert _same(H.get(), want_w.cuda()), what + ("ef wire",)
    assert torch.equal(R.get().view(torch.int32), want_r.view(torch.int32).cuda()), what + ("ef r",)
    assert H.intact() and R.intact() and torch.equal(W.raw, before), what + ("ef",)
    plan.close()
    # stochastic rounding: segment i under key KEY + i
    H.reset()
    plan = red.cast_plan([(w, h, n, SrKey(KEY + i))
                          for i, (w, h, n) in enumerate(zip(W.ptrs, H.ptrs, counts))],
                         from_torch(F32), from_torch(wire))
    plan.compress(stream=cur, step=STEP)
    rnd = sr.sr_bf16 if wire_name == "bf16" else sr.sr_fp16
    want = _tensor(rnd(g.numpy(), _sr_bits(segs)), wire)
    assert _same(H.get(), want.cuda()), what + ("sr",)
    assert H.intact() and torch.equal(W.raw, before), what + ("sr",)
    plan.close()


def run_pair(red, wire_name, wide_name, u):
    """Both entries, each to its first mismatch: they run different kernels."""
    failed = []
    for entry in (run_single, run_plan):
        try:
            entry(red, wire_name, wide_name, u)
        except AssertionError as e:
            failed.append(f"{entry.__name__}: {str(e).splitlines()[0] if str(e) else e!r}")
    assert not failed, failed


# ------------------------------------------------------------------- tests --
@pytest.fixture(scope="module")
def red():
    assert torch.cuda.is_available()
    return GpuReducer(device=0)


def _line(env, u, *what):
    return f"cast tiles passed: {env} u={u} " + "-".join(what)


def _lines(env):
    out = []
    for u in cs.ENVS[env][3]:
        out += [_line(env, u, w, x) for w, x in PAIRS]
        if u > 1:
            out += [_line(env, u, w, "ef", "sr") for w in cs.WIRES]
    return out


@pytest.mark.parametrize("u", cs.ENVS["default"][3])
@pytest.mark.parametrize("wire,wide", PAIRS, ids=["-".join(p) for p in PAIRS])
def test_write_through_one_and_two_units(red, wire, wide, u):
    """The default tuning: U 1 and 2, every launch write-through."""
    assert not set(cs.ENVS["nt"][0]) & set(os.environ) and "BPSR_COPY_VPT" not in os.environ
    run_pair(red, wire, wide, u)


@pytest.mark.parametrize("wire", cs.WIRES)
def test_write_through_error_feedback_and_stochastic_two_units(red, wire):
    run_ef_sr(red, wire, 2)


@pytest.mark.parametrize("env", ["u4wt", "nt", "u4nt"])
def test_in_a_child_process(env):
    """U 4 write-through; U 1 and 2 non-temporal; U 4 non-temporal.  One child
    a test, so one GPU process at a time; each prints a line per group."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), env],
                       env=dict(os.environ, **cs.ENVS[env][0]), cwd=ROOT, capture_output=True,
                       text=True, timeout=200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = r.stdout.splitlines()
    for line in _lines(env):
        assert line in got, line


if __name__ == "__main__":
    _env = sys.argv[1]
    for _k in ("BPSR_COPY_VPT", "BPSR_WT_MAX_MIB"):
        assert os.environ.get(_k) == cs.ENVS[_env][0].get(_k), _k
    _red = GpuReducer(device=0)
    for _u in cs.ENVS[_env][3]:
        for _w, _x in PAIRS:
            run_pair(_red, _w, _x, _u)
            print(_line(_env, _u, _w, _x), flush=True)
        if _u > 1:
            for _w in cs.WIRES:
                run_ef_sr(_red, _w, _u)
                print(_line(_env, _u, _w, "ef", "sr"), flush=True)
