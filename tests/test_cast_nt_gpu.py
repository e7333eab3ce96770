"""The cast kernels' non-temporal store instantiations (the `POL = kPolNt` half
of prophet_amd/csrc/bpsr_cast_single.h's and bpsr_cast_plan.h's kernels) bit
for bit against the host definitions.

A launch stores write-through below Tuning::wt_max_bytes of output (96 MiB)
and non-temporal from there on, so the short launches of the other cast tests
only ever run the write-through kernels.  The tuning is read once a process:
this file, run as a script in a child process with BPSR_WT_MAX_MIB=0, takes
the non-temporal policy for every launch, and checks for both wires the plain
compress, the decompress with divisors 1 and 8, the error-feedback compress
(wire and residual) and the stochastic-rounding compress, each as the
one-tensor call and as a plan of that segment plus a short one, at one unit a
lane (short launches) and two (2048 such tiles).  A second child with
BPSR_COPY_VPT=4 besides runs four units a lane.  The expected values are the
other tests' host definitions: torch's CPU casts and ``div_`` on the wire
tensor, the four error-feedback lines, prophet_amd/sr.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, ROOT)

from prophet_amd import sr  # noqa: E402
from prophet_amd.dtypes import DType  # noqa: E402
from prophet_amd.reducer import GpuReducer, SrKey  # noqa: E402

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.timeout(240)]

F32 = DType.FLOAT32
WIRES = [(DType.FLOAT16, torch.float16, "fp16"), (DType.BFLOAT16, torch.bfloat16, "bf16")]
# Launches below 2048 tiles run tiles of 256 lanes x 8 elements x 1 unit per lane
TILE = 256 * 8
GUARD = 64      # bytes
SHORT = 37      # elements of a plan's second segment
KEY, KEY2, STEP = 0x1234abcd, 77, 5


def _child(env):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=dict(os.environ, **env),
                       cwd=ROOT, capture_output=True, text=True, timeout=100)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r.stdout


def test_nt_store_kernels_in_child_processes():
    """Two children, one after the other (one GPU process at a time): one and
    two units a lane, then four."""
    assert "nt case passed: units 1 2" in _child({"BPSR_WT_MAX_MIB": "0"})
    assert "nt case passed: units 4" in _child({"BPSR_WT_MAX_MIB": "0", "BPSR_COPY_VPT": "4"})


# ---------------------------------------------------------------- the child --
class _Buf:
    """`nbytes` of device memory `off` bytes past a 256-byte boundary, between
    0xA5 guard bytes."""

    def __init__(self, nbytes, off, dt, fill=None):
        self.raw = torch.empty(nbytes + 1024, dtype=torch.uint8, device="cuda")
        self.raw.fill_(0xA5)
        self.lo = (-self.raw.data_ptr()) % 256 + 256 + off
        self.hi = self.lo + nbytes
        self.t = self.raw[self.lo:self.hi].view(dt)
        if fill is not None:
            self.t.copy_(fill)

    def intact(self):
        return bool((self.raw[self.lo - GUARD:self.lo] == 0xA5).all()) and \
            bool((self.raw[self.hi:self.hi + GUARD] == 0xA5).all())


def _same(buf, want):
    """The buffer holds the bits of the host tensor `want`, its guards intact."""
    ib = {2: torch.int16, 4: torch.int32}[want.element_size()]
    return buf.intact() and torch.equal(buf.t.view(ib), want.view(ib).cuda())


def host_ef(g, r, wire):
    """tests/test_compress_ef_gpu.py's host definition: (w, r')."""
    c = g + r
    w = c.to(wire)
    b = w.to(torch.float32)
    return w, torch.where(torch.isfinite(b), c - b, torch.zeros_like(c))


def _data(n, seed):
    """Finite f32 over fp16's and bf16's ranges and past them (no NaN: every
    expected bit is compared), and residuals of about a wire step."""
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(n) * np.exp2(rng.integers(-30, 20, n))).astype(np.float32)
    r = g * np.float32(2.0 ** -10) * rng.choice(np.float32([-1.0, 1.0]), n)
    return torch.from_numpy(g), torch.from_numpy(r)


def _case(red, n, k):
    """Every cast of `n` elements, the wide side (and the residual) k f32
    elements and the wire side k wire elements past a 16-byte boundary: for
    k = 1 they co-align after a head of 7."""
    g, r = _data(n, 100 + n % 1000 + k)
    gs, rs = _data(SHORT, 7)
    r16, r16s = sr.sr_bits(n, KEY, STEP), sr.sr_bits(SHORT, KEY2, STEP)
    x, xs = _Buf(n * 4, k * 4, torch.float32, g), _Buf(SHORT * 4, 0, torch.float32, gs)

    def outs(width, dt, fill=(None, None)):
        return _Buf(n * width, k * width, dt, fill[0]), _Buf(SHORT * width, 0, dt, fill[1])

    for wd, wt, name in WIRES:
        tag = (n, k, name)
        # plain compress: the one-tensor call, then the plan over its own wide copy
        want_h, want_hs = g.to(wt), gs.to(wt)
        h, _ = outs(2, wt)
        red.compress(h.t, x.t, n, F32, wd)
        assert _same(h, want_h), tag
        px, pxs = outs(4, torch.float32, (g, gs))
        ph, phs = outs(2, wt)
        plan = red.cast_plan([(px.t, ph.t, n), (pxs.t, phs.t, SHORT)], F32, wd)
        plan.compress()
        assert _same(ph, want_h) and _same(phs, want_hs), tag
        assert _same(px, g) and _same(pxs, gs), tag
        # decompress: the divide is on the wire value, rounded to the wire format
        for d in (1, 8):
            want_x = (want_h.clone().div_(d) if d > 1 else want_h).to(torch.float32)
            want_xs = (want_hs.clone().div_(d) if d > 1 else want_hs).to(torch.float32)
            o, _ = outs(4, torch.float32)
            red.decompress(o.t, h.t, n, F32, wd, d)
            assert _same(o, want_x), tag + (d,)
            px.t.fill_(-1.0)
            pxs.t.fill_(-1.0)
            plan.decompress(d)
            assert _same(px, want_x) and _same(pxs, want_xs), tag + (d,)
            assert _same(ph, want_h) and _same(phs, want_hs), tag + (d,)
        plan.close()
        # error feedback: wire and residual
        want_w, want_r = host_ef(g, r, wt)
        want_ws, want_rs = host_ef(gs, rs, wt)
        res, _ = outs(4, torch.float32, (r, rs))
        h, _ = outs(2, wt)
        red.compress_ef(h.t, res.t, x.t, n, F32, wd)
        assert _same(h, want_w) and _same(res, want_r), tag
        res, ress = outs(4, torch.float32, (r, rs))
        h, hs = outs(2, wt)
        plan = red.cast_plan([(x.t, h.t, n, res.t), (xs.t, hs.t, SHORT, ress.t)], F32, wd)
        plan.compress()
        assert _same(h, want_w) and _same(res, want_r), tag
        assert _same(hs, want_ws) and _same(ress, want_rs), tag
        plan.close()
        # stochastic rounding: element i under 16 bits of Philox(i >> 2, step, key)
        rnd = sr.sr_bf16 if name == "bf16" else sr.sr_fp16
        want_s = torch.from_numpy(rnd(g.numpy(), r16).view(np.int16))
        want_ss = torch.from_numpy(rnd(gs.numpy(), r16s).view(np.int16))
        h, _ = outs(2, wt)
        red.compress_sr(h.t, x.t, n, KEY, STEP, wd)
        assert _same(h, want_s), tag
        h, hs = outs(2, wt)
        plan = red.cast_plan([(x.t, h.t, n, SrKey(KEY)), (xs.t, hs.t, SHORT, SrKey(KEY2))],
                             F32, wd)
        plan.compress(step=STEP)
        assert _same(h, want_s) and _same(hs, want_ss), tag
        plan.close()
    assert _same(x, g) and _same(xs, gs)


def _big(units):
    """tests/test_compress_sr_gpu.py:_big_case's shape: 2048 full tiles of
    `units` units a lane, a partial tile, a head of 7 and a tail."""
    return 2048 * units * TILE + TILE + 7 + 5


if __name__ == "__main__":
    assert os.environ.get("BPSR_WT_MAX_MIB") == "0"
    red = GpuReducer(device=0)
    if os.environ.get("BPSR_COPY_VPT") == "4":
        _case(red, _big(4), 1)
        print("nt case passed: units 4")
    else:
        for n in (5, TILE - 1, TILE + 9, 3 * 8192 + 13):
            for k in (0, 1):
                _case(red, n, k)
        _case(red, _big(2), 1)
        print("nt case passed: units 1 2")
