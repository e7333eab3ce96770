"""Gradient compression for push_pull (the byteps/torch ``Compression`` surface).

``Compression.none`` and ``Compression.fp16`` keep the reference's interface
(byteps/torch/compression.py): ``compress(tensor) -> (compressed, ctx)`` and
``decompress(tensor, ctx)``, with ``ctx`` the original dtype.  The fp16
compressor casts floating tensors to fp16 before the push and back after the
pull; everything else (integers, tensors that are fp16 already) passes
through as the same object.

``Compression.bf16`` is the build's own second wire format with the same
surface: floating tensors travel as bf16, which has f32's exponent range — a
sum of gradients that fp16 turns into inf (from 65,520 up) stays finite.  The
casts are pinned to torch's CPU casts (round to nearest even, f32 subnormals
kept, f64 through f32); on the device they are
``torch.ops.bpsr.compress_bf16*`` / ``decompress_bf16_out``
(``prophet_amd/csrc/bpsr_k_cast_bf16.hip``).  A numpy bf16 buffer is raw
``uint16`` bits (``dtypes.numpy_dtype``).

Where the casts run:

* CUDA tensors: the HIP kernels of ``prophet_amd/csrc/bpsr_k_cast.hip``
  through ``torch.ops.bpsr.compress_fp16*`` / ``decompress_fp16_out``, on the
  current stream of the tensor's device, so they order with the caller's
  torch work.  There is no torch fallback on the device.
* CPU tensors and numpy arrays: torch's host casts, which is the reference's
  own path (``tensor.type(torch.float16)``) and the semantics the kernels are
  pinned to bit for bit.

``decompress_into(out, compressed, divisor)`` is the fused form push_pull
uses: with ``divisor > 1`` the fp16 value is divided and rounded to fp16
FIRST and widened afterwards — the reference's ``average=True`` divides the
compressed tensor in place (byteps/torch/ops.cc:77-81) before it is
decompressed (byteps/torch/__init__.py:166-170).

``compress_many_into`` / ``decompress_many_into`` are the same casts for a
whole iteration's tensors: the device tensors are grouped by (device, wide
dtype) and each group is ONE launch of a cast plan
(``byteps_reduce_cast_plan_*``, ``prophet_amd/csrc/bpsr_k_cast_plan.hip``) on
the calling thread's current stream of that device; per tensor the bytes are
those of ``compress_into`` / ``decompress_into``.  A :class:`CastPlanCache`
keeps the plans between iterations.  There is no ``torch.library`` op for
plans: a plan owns raw device pointers, which a traced graph cannot — the
one-tensor ops stay the traceable form.

``Compression.fp16_ef`` / ``Compression.bf16_ef`` add error feedback to the
two wire formats, which are memoryless otherwise: whatever the 2-byte
rounding drops in an iteration is gone (on the fp16 wire an f32 gradient
below 2^-25 is sent as zero forever; bf16 keeps 8 significant bits a step).
A per-tensor f32 residual ``r`` holds what the wire could not carry and is
added back before the next cast.  Per element, float32 tensors only::

    c  = g + r                                    # f32 add
    w  = wire(c)                                  # the plain compress
    b  = w.float()                                # exact
    r' = torch.where(torch.isfinite(b), c - b, 0) # exact where finite; never non-finite

``compress_ef_into(out, residual, tensor)`` writes ``w`` and replaces ``r``
in place — device tensors in one pass of
``torch.ops.bpsr.compress_<wire>_ef_out``
(``prophet_amd/csrc/bpsr_cast_ef.h``), CPU tensors and numpy arrays through
the four torch lines above, which is the semantics the kernels are pinned to
bit for bit.  ``compress_many_ef_into`` is the cast-plan form.  The wire
carries ordinary fp16 / bf16, so the server, the folds and ``decompress*``
are those of the plain compressors.  The stateless ``compress(tensor)`` stays
the plain cast: it has no residual to read or to leave the error in.
Tensors other than float32 (f64 and the 2-byte floats included) pass through
uncompressed, as integers do.

``Compression.fp16_sr`` / ``Compression.bf16_sr`` remove the same bias without
any state: stochastic rounding.  A float32 value is rounded up with a
probability equal to the fraction the wire format drops, so what is delivered
is right in expectation (a gradient of ``1 + 2^-12`` on the bf16 wire is sent
as ``1 + 2^-7`` one time in 32, not as ``1.0`` forever).  The wire value is a
pure function of the value's bits, a ``key``, a ``step`` and the element's
index — Philox2x32-10 bits, no RNG state — defined by the numpy lines of
``prophet_amd/sr.py``.  ``compress_sr_into(out, tensor, key, step)`` writes
it: device tensors in one pass of ``torch.ops.bpsr.compress_<wire>_sr_out``
(the rounding scheme of ``prophet_amd/csrc/bpsr_cast_sr.h`` in the plain
compress's kernel, 6 bytes an element like it), CPU tensors and numpy arrays through ``sr.py`` itself, bit for bit
the same.  ``compress_many_sr_into`` is the cast-plan form, one ``step`` for
the launch and one key per tensor.  A caller never uses a ``(key, step)`` pair
twice.  ``compress(tensor)`` stays the plain cast, ``decompress*`` is
inherited, and tensors other than float32 pass through, as for error
feedback.  Not covered: the server's fold still rounds its sum to the wire
format to nearest even, so stochastic rounding makes the worker's cast
unbiased, not the whole round.

``decompress_into(..., stats=)`` / ``decompress_many_into(..., stats=)`` also
report, per tensor, two numbers computed from exactly the values the
decompress writes: the sum of the squares of the finite ones, added up in
float64, and the count of the others (+-inf, NaN) — what a global-norm clip
and a GradScaler-style overflow check need, without a second sweep over the
gradients.  :func:`decompress_stats` below is the definition; the order of the
additions is the implementation's.  Device tensors go through the cast plan's
``STATS`` decompress (``byteps_reduce_cast_plan_decompress_stats``, DESIGN.md
§11.5): the plain decompress's bytes, the statistics from the registers that
hold them, then a small kernel that adds each tensor's partial sums up.  The
rows land in a float64 device tensor in stream order; nothing synchronises
with the host.

``decompress_many_into(..., clip_norm=, clip_eps=, unscale=)`` clips by the
global norm and unscales INSIDE the decompress, in three
launches on one stream: ``measure_many_with`` takes the statistics of the
values the decompress would write and writes none of them
(``byteps_reduce_cast_plan_measure``: the 2-byte side is read, the gradients are
not touched), ``GpuReducer.clip_record`` turns the rows into the norm and the
multipliers (:func:`clip_record` below is the definition), and
``decompress_many_with(..., scale=)`` writes every value times ``mult``
(``byteps_reduce_cast_plan_decompress_scaled``) — so an unclipped gradient is
never written and no pass reads the gradients again.  The record is returned;
for device tensors it stays on the device.

``apply_sgd_many(params, compressed, momenta, divisor, lr=, ...)`` goes one
step further: the SGD step itself runs inside the
decompress.  One launch per device reads the wire, the float32 parameter and
its momentum buffer and writes the last two in place — 18 bytes an element,
against 6 for the scaled decompress plus 20 for a fused optimizer — and the
gradient is never written.  ``prophet_amd/sgd.py`` is the definition, bit for
bit.  With ``record=`` the gradient is multiplied by the clip record's
``mult`` first, and with ``skip_nonfinite`` a record that counted a
non-finite value leaves parameters and momenta untouched, decided on the
device (GradScaler's skipped step with no host synchronisation).  There is no
``torch.library`` op for it either: an SGD plan owns raw device pointers.

``Compression.onebit_ef`` leaves the 2-byte wires behind:
a float32 tensor travels as one bit an element plus one float32 scale, the
mean of ``|tensor + residual|``, 32x smaller than float32, with error
feedback.  ``prophet_amd/onebit.py`` is the definition.  A payload is a flat
uint8 buffer (``payload_like``); ``compress_many_ef_into`` is three launches
per device, ``fold_many_into`` decodes up to 16 payloads per output and adds
them in order in one.  The PS server cannot fold a packed payload, so
``Worker.init_tensor`` refuses this compressor.

``Compression.topk_ef`` is the sparsifier beside it: a
float32 tensor travels as the ``k`` values of largest ``|tensor + residual|``
with their indices, ``16 + 8 k`` bytes, and the rest waits in the residual.
``prophet_amd/topk.py`` is the definition, byte for byte: a radix select, a
deterministic tie rule (the lowest indices win) and no floating-point
reduction.  ``payload_like(tensor, ratio)`` sizes the payload, which carries
its ``k`` in its size; ``compress_many_ef_into`` is one fixed sequence of
launches per device, ``fold_many_into`` adds up to 16 sparse payloads per
output in one.  Its server round is opt-in and needs a ratio (DESIGN.md
§11.18): ``Compression.topk_ef.at(ratio)`` named in a front end's
``packed_wires``, ``refold_many_into`` on the store; without a ratio
``Worker.init_tensor`` refuses this compressor over every front end.

``Compression.mxfp8_ef`` and ``Compression.mxfp4_ef`` sit between the 2-byte
wires and those two: every 32 consecutive elements share one
power-of-two scale byte and travel as OCP e4m3 or e2m1 codes, 8.25 or 4.25 bits
an element, the rounding and saturation error waiting in the residual.
``prophet_amd/mx.py`` is the definition, byte for byte: an integer block
maximum, round to nearest even, no floating-point reduction.
``compress_many_ef_into`` is ONE launch per device, ``fold_many_into`` decodes
up to 16 payloads per output and adds them in order in one.  There is no server
round for them yet: ``Worker.init_tensor`` refuses both over every front end.

``Compression.mxfp8_sr`` and ``Compression.mxfp4_sr`` are the same wire with no
residual (``prophet_amd/mx_sr.py`` is the definition): the
codes are rounded stochastically under ``fp16_sr``'s bits and the scale is
bumped so that nothing is clamped, which makes the decode right in expectation.
``Compression.mxfp8_rht_sr`` and ``Compression.mxfp4_rht_sr`` rotate every whole
block by a random-sign Hadamard transform first, under a key all workers share,
and undo it once in the fold.  ``compress_many_sr_into`` and ``fold_many_into``
are ONE launch per device each; ``Worker.init_tensor`` refuses all four.

All six block-scaled wires take float16 and bfloat16 tensors as well as float32
(DESIGN.md §11.16): a half gradient gives the payload of its exact float32
upcast, the residual stays float32, and ``fold_many_into`` writes float32,
float16 or bfloat16 outputs, converting its float32 result once.  Segments are
grouped by device and dtype, ONE launch a group.

``Compression.powersgd_ef`` is the low-rank wire: a float32
tensor of two or more dimensions is an n x m matrix and travels as ``P`` (n x r)
and ``Q`` (m x r), ``(n + m) r`` floats, with error feedback and a warm-started
``Q``.  ``prophet_amd/powersgd.py`` is the definition.  It is the first wire
whose device path is not pinned byte for byte throughout: the two projections
run on f32 matrix instructions in the kernels' own order and are held to a dot
product's error bound; the ``g + R`` left in the residual, all of ``finish`` and
determinism are pinned.  ``P`` and ``Q`` are plain float32 tensors, so the round
needs no compressed context: ``powersgd.push_pull_many`` sends them with
``Compression.none`` between the four phases ``project_p_many``,
``orthogonalize_many``, ``project_q_many`` and ``finish_many``.
``Worker.init_tensor`` refuses the compressor itself.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from .reducer import SrKey


def _is_torch(x) -> bool:
    return hasattr(x, "data_ptr")


def _is_floating(x) -> bool:
    if _is_torch(x):
        return bool(x.dtype.is_floating_point)
    return bool(np.issubdtype(x.dtype, np.floating))


def _is_half(x) -> bool:
    if _is_torch(x):
        import torch
        return x.dtype == torch.float16
    return x.dtype == np.float16


def _is_bf16(x) -> bool:
    """torch bf16; numpy has no bf16 (its raw uint16 bits are integers and are
    not compressed either)."""
    if _is_torch(x):
        import torch
        return x.dtype == torch.bfloat16
    return False


def _on_device(x) -> bool:
    return _is_torch(x) and x.device.type == "cuda"


def _as_host_tensor(x):
    """A CPU torch view of a CPU tensor or numpy array (no copy)."""
    import torch
    return x if _is_torch(x) else torch.from_numpy(x)


def _as_host_bf16(x):
    """The same for a bf16 buffer: a numpy one carries raw uint16 bits."""
    import torch
    return x if _is_torch(x) else torch.from_numpy(x.view(np.int16)).view(torch.bfloat16)


def decompress_stats(out):
    """The decompress statistics of one output, the pinned definition:
    ``(sum of squares of the finite values in float64, count of the
    non-finite ones)`` of a CPU tensor or numpy array."""
    if _is_torch(out):
        import torch
        x = out.detach().reshape(-1).to(torch.float64).numpy()
    else:
        x = out.reshape(-1).astype(np.float64)
    fin = np.isfinite(x)
    return float(np.square(x[fin]).sum()), int(np.count_nonzero(~fin))


class ClipValues:
    """A clip record on the host (:func:`clip_record`): ``sumsq``,
    ``nonfinite``, ``norm`` as float64, ``coef``, ``mult`` as float32;
    ``found_inf`` is ``nonfinite``."""

    def __init__(self, sumsq, nonfinite, norm, coef, mult):
        self.sumsq, self.nonfinite, self.norm = sumsq, nonfinite, norm
        self.coef, self.mult = coef, mult
        self.found_inf = nonfinite


def clip_record(rows, max_norm: float, eps: float = 1e-6, inv_scale=None) -> ClipValues:
    """The clip record of statistics rows, the pinned definition
    (``byteps_reduce_clip_record``): ``rows`` is float64 ``[n, 2]`` (or ``2 n``)
    of ``(sumsq, nonfinite)`` on the host, ``inv_scale`` a number or None (1).
    The order of the additions of ``sumsq`` is the implementation's."""
    if not max_norm > 0 or not np.isfinite(max_norm):
        raise ValueError(f"max_norm {max_norm} is not a finite positive number")
    if not eps >= 0:
        raise ValueError(f"eps {eps} < 0")
    if _is_torch(rows):
        rows = rows.detach().numpy()
    r = np.asarray(rows, dtype=np.float64).reshape(-1, 2)
    sumsq = np.float64(r[:, 0].sum())
    nonfinite = np.float64(r[:, 1].sum())
    inv = np.float64(1.0) if inv_scale is None else np.float64(np.float32(inv_scale))
    norm = np.sqrt(sumsq) * inv
    with np.errstate(divide="ignore"):    # all-zero gradients, eps 0: +inf, c = 1
        q = np.float64(max_norm) / (norm + np.float64(eps))
    c = q if q < 1.0 else np.float64(1.0)
    return ClipValues(sumsq, nonfinite, norm, np.float32(c), np.float32(c * inv))


def _scale_host_(out, m) -> None:
    """``out *= m`` on the host under the scaled decompress's rounding: the
    f32 product for f32 and, before the cast back, for the 2-byte types; the
    f64 product for f64."""
    import torch
    t = _as_host_tensor(out)
    m32 = torch.tensor(float(np.float32(m)), dtype=torch.float32)
    if t.dtype == torch.float64:
        t.mul_(m32.to(torch.float64))
    elif t.dtype == torch.float32:
        t.mul_(m32)
    else:
        t.copy_((t.to(torch.float32) * m32).to(t.dtype))


def _empty_like(x):
    if _is_torch(x):
        import torch
        return torch.empty_like(x)
    return np.empty_like(x)


def _check_stats(stats, shape) -> None:
    """``stats``: a float64 tensor or array of ``shape``."""
    if _is_torch(stats):
        import torch
        ok = stats.dtype == torch.float64
    else:
        ok = isinstance(stats, np.ndarray) and stats.dtype == np.float64
    if not ok:
        raise ValueError(f"stats must be a float64 tensor or array, got "
                         f"{getattr(stats, 'dtype', type(stats))}")
    if tuple(stats.shape) != tuple(shape):
        raise ValueError(f"stats must have shape {tuple(shape)}, got {tuple(stats.shape)}")


class CastPlanCache:
    """The cast plans of the last few iterations, least recently used out
    first.  A plan is found again by its wide dtype, its wire dtype and the
    (wide address, 2-byte address, element count) of every segment, so a tensor that moved
    misses and gets a new plan.  An error-feedback plan's segments carry
    their residual's address as well: a moved residual misses too, and the
    plan over the same tensors without residuals is another plan.  A cached plan holds its tensors: their
    memory cannot be freed, so no other tensor can appear at a cached
    address while the plan that names it is alive.  A stochastic-rounding
    plan's segments carry their key (``SrKey``): another key misses, and the
    plain plan over the same tensors is another plan."""

    def __init__(self, capacity: int = 4):
        self.capacity = int(capacity)
        self.built = 0                    # plans created so far
        self._plans: OrderedDict = OrderedDict()

    def __len__(self) -> int:
        return len(self._plans)

    def get(self, wide_dtype: int, pairs, wire_dtype: int = 2):
        """The plan over ``pairs`` of flat ``(wide, half)`` device tensors on
        the current device, built on a miss.  ``wire_dtype``: the dtype of
        the ``half`` side (``DType.FLOAT16`` unless named).  Items of three,
        ``(wide, half, residual)``, ask for the error-feedback plan, and
        ``(wide, half, SrKey(key))`` for the stochastic-rounding plan."""
        key = (int(wide_dtype), int(wire_dtype)) + tuple(
            (int(p[0].data_ptr()), int(p[1].data_ptr()), int(p[0].numel()))
            + tuple(("sr", int(r)) if isinstance(r, SrKey) else int(r.data_ptr()) for r in p[2:])
            for p in pairs)
        return self._get(key, lambda: _new_plan(wide_dtype, pairs, wire_dtype))

    def _get(self, key, build):
        """The plan under ``key``, made by ``build()`` on a miss."""
        plan = self._plans.get(key)
        if plan is not None:
            self._plans.move_to_end(key)
            return plan
        plan = build()
        self.built += 1
        self._plans[key] = plan
        while len(self._plans) > self.capacity:
            _, old = self._plans.popitem(last=False)
            old.close()                   # waits for its launches in flight
        return plan

    def get_sgd(self, triples, wire_dtype: int = 2):
        """The SGD plan (``GpuReducer.sgd_plan``) over ``triples`` of flat
        ``(param, half, momentum)`` device tensors on the current device, built
        on a miss.  Its key is marked: the error-feedback plan over the same
        three addresses is another plan."""
        key = ("sgd", int(wire_dtype)) + tuple(
            (int(p.data_ptr()), int(h.data_ptr()), int(p.numel()), int(m.data_ptr()))
            for p, h, m in triples)
        return self._get(key, lambda: _new_sgd_plan(triples, wire_dtype))

    def get_onebit(self, segs):
        """The 1-bit compress plan (``GpuReducer.onebit_plan``) over ``segs`` of
        flat ``(grad, resid, payload)`` device tensors on the current device."""
        key = ("onebit",) + tuple(
            (int(g.data_ptr()), int(r.data_ptr()), int(p.data_ptr()), int(g.numel()))
            for g, r, p in segs)
        return self._get(key, lambda: _new_onebit_plan(segs))

    def get_onebit_fold(self, segs, nsrc: int):
        """The 1-bit fold plan (``GpuReducer.onebit_fold_plan``) over ``segs`` of
        ``(out, payloads)`` device tensors on the current device."""
        key = ("onebit_fold", int(nsrc)) + tuple(
            (int(o.data_ptr()), int(o.numel())) + tuple(int(p.data_ptr()) for p in ps)
            for o, ps in segs)
        return self._get(key, lambda: _new_onebit_fold_plan(segs, nsrc))

    def get_onebit_refold(self, segs, nsrc: int):
        """The 1-bit refold plan (``GpuReducer.onebit_refold_plan``) over
        ``segs`` of ``(payloads, resid, out_payload)`` device tensors on the
        current device."""
        key = ("onebit_refold", int(nsrc)) + tuple(
            (int(r.data_ptr()), int(o.data_ptr()), int(r.numel()))
            + tuple(int(p.data_ptr()) for p in ps) for ps, r, o in segs)
        return self._get(key, lambda: _new_onebit_refold_plan(segs, nsrc))

    def get_topk(self, segs):
        """The top-k compress plan (``GpuReducer.topk_plan``) over ``segs`` of
        flat ``(grad, resid, payload)`` device tensors on the current device;
        ``k`` is the payload's (``topk.k_of``), so another ratio misses."""
        key = ("topk",) + tuple(
            (int(g.data_ptr()), int(r.data_ptr()), int(p.data_ptr()), int(g.numel()),
             int(p.numel())) for g, r, p in segs)
        return self._get(key, lambda: _new_topk_plan(segs))

    def get_topk_fold(self, segs, nsrc: int):
        """The top-k fold plan (``GpuReducer.topk_fold_plan``) over ``segs`` of
        ``(out, payloads)`` device tensors on the current device."""
        key = ("topk_fold", int(nsrc)) + tuple(
            (int(o.data_ptr()), int(o.numel()), int(ps[0].numel()))
            + tuple(int(p.data_ptr()) for p in ps) for o, ps in segs)
        return self._get(key, lambda: _new_topk_fold_plan(segs, nsrc))

    def get_topk_refold(self, segs, nsrc: int):
        """The top-k refold plan (``GpuReducer.topk_refold_plan``) over ``segs``
        of ``(payloads, resid, out_payload)`` device tensors on the current
        device; ``k`` is the output payload's (``topk.k_of``)."""
        key = ("topk_refold", int(nsrc)) + tuple(
            (int(r.data_ptr()), int(o.data_ptr()), int(r.numel()), int(o.numel()))
            + tuple(int(p.data_ptr()) for p in ps) for ps, r, o in segs)
        return self._get(key, lambda: _new_topk_refold_plan(segs, nsrc))

    def get_mx(self, segs, fmt: str, dtype: int = 0):
        """The block-scaled compress plan (``GpuReducer.mx_plan``) over ``segs``
        of flat ``(grad, resid, payload)`` device tensors on the current device,
        the gradients of ``dtype`` (a DType id; float32 unless named)."""
        key = ("mx", fmt, int(dtype)) + tuple(
            (int(g.data_ptr()), int(r.data_ptr()), int(p.data_ptr()), int(g.numel()))
            for g, r, p in segs)
        return self._get(key, lambda: _new_mx_plan(segs, fmt, dtype))

    def get_mx_fold(self, segs, nsrc: int, fmt: str, dtype: int = 0):
        """The block-scaled fold plan (``GpuReducer.mx_fold_plan``) over ``segs``
        of ``(out, payloads)`` device tensors on the current device, the
        outputs of ``dtype``."""
        key = ("mx_fold", fmt, int(nsrc), int(dtype)) + tuple(
            (int(o.data_ptr()), int(o.numel())) + tuple(int(p.data_ptr()) for p in ps)
            for o, ps in segs)
        return self._get(key, lambda: _new_mx_fold_plan(segs, nsrc, fmt, dtype))

    def get_mx_refold(self, segs, nsrc: int, fmt: str):
        """The block-scaled refold plan (``GpuReducer.mx_refold_plan``) over
        ``segs`` of ``(payloads, resid, out_payload)`` device tensors on the
        current device."""
        key = ("mx_refold", fmt, int(nsrc)) + tuple(
            (int(r.data_ptr()), int(o.data_ptr()), int(r.numel()))
            + tuple(int(p.data_ptr()) for p in ps) for ps, r, o in segs)
        return self._get(key, lambda: _new_mx_refold_plan(segs, nsrc, fmt))

    def get_mx_sr(self, segs, fmt: str, rotate: bool = False, dtype: int = 0):
        """The stateless block-scaled compress plan (``GpuReducer.mx_sr_plan``)
        over ``segs`` of flat ``(grad, payload, key, rot_key)`` device tensors
        and keys on the current device, the gradients of ``dtype``: another key
        misses."""
        key = ("mx_sr", fmt, bool(rotate), int(dtype)) + tuple(
            (int(g.data_ptr()), int(p.data_ptr()), int(g.numel()), int(k), int(rk))
            for g, p, k, rk in segs)
        return self._get(key, lambda: _new_mx_sr_plan(segs, fmt, rotate, dtype))

    def get_mx_rht_fold(self, segs, nsrc: int, fmt: str, dtype: int = 0):
        """The rotated block-scaled fold plan (``GpuReducer.mx_rht_fold_plan``)
        over ``segs`` of ``(out, payloads, rot_key)`` on the current device,
        the outputs of ``dtype``."""
        key = ("mx_rht_fold", fmt, int(nsrc), int(dtype)) + tuple(
            (int(o.data_ptr()), int(o.numel()), int(rk)) + tuple(int(p.data_ptr()) for p in ps)
            for o, ps, rk in segs)
        return self._get(key, lambda: _new_mx_rht_fold_plan(segs, nsrc, fmt, dtype))

    def get_powersgd(self, segs, rank: int):
        """The PowerSGD plan (``GpuReducer.powersgd_plan``) over ``segs`` of
        ``(grad, resid, p, q, qn, out, n, m)`` device tensors and shapes on the
        current device."""
        key = ("powersgd", int(rank)) + tuple(
            tuple(int(x.data_ptr()) for x in s[:6]) + (int(s[6]), int(s[7])) for s in segs)
        return self._get(key, lambda: _new_powersgd_plan(segs, rank))

    def close(self) -> None:
        while self._plans:
            _, plan = self._plans.popitem(last=False)
            plan.close()


def _new_powersgd_plan(segs, rank: int):
    from .torch_ops import _red
    return _red().powersgd_plan(segs, rank)


def _new_mx_plan(segs, fmt: str, dtype: int = 0):
    from .torch_ops import _red
    return _red().mx_plan([(g, r, p, int(g.numel())) for g, r, p in segs], fmt, dtype)


def _new_mx_fold_plan(segs, nsrc: int, fmt: str, dtype: int = 0):
    from .torch_ops import _red
    return _red().mx_fold_plan([(o, ps, int(o.numel())) for o, ps in segs], nsrc, fmt, dtype)


def _new_mx_refold_plan(segs, nsrc: int, fmt: str):
    from .torch_ops import _red
    return _red().mx_refold_plan([(ps, r, o, int(r.numel())) for ps, r, o in segs], nsrc, fmt)


def _new_mx_sr_plan(segs, fmt: str, rotate: bool, dtype: int = 0):
    from .torch_ops import _red
    return _red().mx_sr_plan([(g, p, int(g.numel()), k, rk) for g, p, k, rk in segs], fmt, rotate,
                             dtype)


def _new_mx_rht_fold_plan(segs, nsrc: int, fmt: str, dtype: int = 0):
    from .torch_ops import _red
    return _red().mx_rht_fold_plan([(o, ps, int(o.numel()), rk) for o, ps, rk in segs], nsrc, fmt,
                                   dtype)


def _new_topk_plan(segs):
    from .topk import k_of
    from .torch_ops import _red
    return _red().topk_plan([(g, r, p, int(g.numel()), k_of(p)) for g, r, p in segs])


def _new_topk_fold_plan(segs, nsrc: int):
    from .topk import k_of
    from .torch_ops import _red
    return _red().topk_fold_plan([(o, ps, int(o.numel()), k_of(ps[0])) for o, ps in segs], nsrc)


def _new_topk_refold_plan(segs, nsrc: int):
    from .topk import k_of
    from .torch_ops import _red
    return _red().topk_refold_plan([(ps, r, o, int(r.numel()), k_of(o)) for ps, r, o in segs],
                                   nsrc)


def _new_onebit_plan(segs):
    from .torch_ops import _red
    return _red().onebit_plan([(g, r, p, int(g.numel())) for g, r, p in segs])


def _new_onebit_fold_plan(segs, nsrc: int):
    from .torch_ops import _red
    return _red().onebit_fold_plan([(o, ps, int(o.numel())) for o, ps in segs], nsrc)


def _new_onebit_refold_plan(segs, nsrc: int):
    from .torch_ops import _red
    return _red().onebit_refold_plan([(ps, r, o, int(r.numel())) for ps, r, o in segs], nsrc)


def _new_sgd_plan(triples, wire_dtype: int = 2):
    from .torch_ops import _red
    return _red().sgd_plan([(p, h, int(p.numel()), m) for p, h, m in triples], wire_dtype)


def _new_plan(wide_dtype: int, pairs, wire_dtype: int = 2):
    from .torch_ops import _red
    return _red().cast_plan([(p[0], p[1], int(p[0].numel())) + tuple(p[2:]) for p in pairs],
                            wide_dtype, wire_dtype)


def _cast_many(comp, pairs, compress: bool, divisor: int, plans, extras=None, step=None,
               stats=None, measure: bool = False, scale=None) -> None:
    """``pairs`` of ``(wide, half)`` tensors or arrays cast by compressor
    ``comp``: the device ones as one plan launch per (device, wide dtype, wire
    dtype), the host ones one by one.  ``extras`` (one per pair, as a cast
    plan's segments carry them) name the scheme: with f32 residuals the plans
    are error-feedback plans and the compress is ``compress_ef_into``'s, with
    ``SrKey`` keys they are stochastic-rounding plans and the compress is
    ``compress_sr_into``'s under ``step``; the decompress is the plain one
    through the same plan.  ``stats`` (decompress only): float64
    ``[len(pairs), 2]``, row i the statistics of pair i — a device pair's row
    lives on its device, a host pair's on the host; each plan writes its own
    rows, which are copied to their places in stream order.  ``measure``
    (decompress, with ``stats``): the statistics alone, no wide side is
    written.  ``scale`` (decompress, without ``stats``): every value written is
    multiplied by it — a 1-element float32 device tensor for device pairs, a
    number for host pairs."""
    if int(divisor) < 1:
        raise ValueError(f"divisor {divisor} < 1")
    if measure and (compress or stats is None):
        raise ValueError("measure is a decompress with stats")
    if scale is not None and (compress or stats is not None):
        raise ValueError("scale is a decompress without stats")
    if stats is not None:
        _check_stats(stats, (len(pairs), 2))
    groups: dict = {}
    rows: dict = {}
    for i, (wide, half) in enumerate(pairs):
        extra = None if extras is None else extras[i]
        if not _on_device(wide) and not _on_device(half):
            if compress:
                comp.compress_with(half, wide, extra, step)
            else:
                if stats is not None and _on_device(stats):
                    raise ValueError(f"stats is on {stats.device}, tensor {i} on the host")
                if scale is not None and _is_torch(scale) and _on_device(scale):
                    raise ValueError(f"scale is on {scale.device}, tensor {i} on the host")
                comp.decompress_into(_empty_like(wide) if measure else wide, half, divisor,
                                     **({} if stats is None else {"stats": stats[i]}))
                if scale is not None:
                    _scale_host_(wide, scale.item() if _is_torch(scale) else scale)
            continue
        comp._check_segment(half, wide, extra)
        seg = (wide.reshape(-1), half.reshape(-1)) + (
            () if extra is None else (extra.reshape(-1) if _is_torch(extra) else extra,))
        if stats is not None and (not _on_device(stats) or stats.device != wide.device):
            raise ValueError(f"stats is on {getattr(stats, 'device', 'the host')}, "
                             f"tensor {i} on {wide.device}")
        if scale is not None and (not _on_device(scale) or scale.device != wide.device):
            raise ValueError(f"scale is on {getattr(scale, 'device', 'the host')}, "
                             f"tensor {i} on {wide.device}")
        key = (wide.device, wide.dtype, comp.wire_torch_dtype())
        groups.setdefault(key, []).append(seg)
        rows.setdefault(key, []).append(i)
    if not groups:
        return
    import torch
    from .dtypes import from_torch
    for (device, dtype, wire), segs in groups.items():
        with torch.cuda.device(device):
            plan = plans.get(from_torch(dtype), segs, from_torch(wire)) if plans is not None \
                else _new_plan(from_torch(dtype), segs, from_torch(wire))
            stream = torch.cuda.current_stream(device)
            try:
                if compress:
                    plan.compress(stream=stream, step=step)
                elif stats is None:
                    plan.decompress(int(divisor), stream=stream, scale=scale)
                else:
                    idx = rows[(device, dtype, wire)]
                    whole = idx == list(range(len(pairs))) and stats.is_contiguous()
                    buf = stats.reshape(-1) if whole else \
                        torch.empty(2 * len(idx), dtype=torch.float64, device=device)
                    if measure:
                        plan.measure(int(divisor), stream=stream, stats=buf)
                    else:
                        plan.decompress(int(divisor), stream=stream, stats=buf)
                    if not whole:         # the plan's rows to the caller's order, run by run
                        got, a = buf.view(-1, 2), 0
                        while a < len(idx):
                            b = a + 1
                            while b < len(idx) and idx[b] == idx[b - 1] + 1:
                                b += 1
                            stats[idx[a]:idx[a] + (b - a)].copy_(got[a:b])
                            a = b
            finally:
                if plans is None:
                    plan.close()          # waits for the launch


class Compressor:
    """Interface: compress a tensor, and undo it given the returned context."""

    @staticmethod
    def compress(tensor):
        raise NotImplementedError

    @staticmethod
    def decompress(tensor, ctx):
        raise NotImplementedError

    ERROR_FEEDBACK = False                # compress_ef_into and a residual per tensor
    STOCHASTIC = False                    # compress_sr_into under a key and a step
    PACKED = False                        # the wire is no element-wise dtype (onebit_ef, topk_ef, mx*_ef)
    SERVER_ROUND = False                  # packed, and packed_round.PackedRound can fold it

    @staticmethod
    def compresses(tensor) -> bool:
        """Whether ``compress`` would change this tensor's dtype."""
        return False


class NoneCompressor(Compressor):
    """The default: tensors travel as they are."""

    @staticmethod
    def compress(tensor):
        return tensor, None

    @staticmethod
    def decompress(tensor, ctx):
        return tensor


class _CastCompressor(Compressor):
    """Floating tensors travel in a 2-byte wire format; the two formats differ
    in the names below only.  Tensors already of the wire dtype, and integers,
    pass through as the same object."""

    WIRE_DTYPE = None                     # DType id a compressed context carries
    WIRE = None                           # "float16" / "bfloat16": the torch dtype's name
    NAME = None                           # "fp16" / "bf16": torch.ops.bpsr.compress_<NAME>*
    NUMPY = None                          # numpy dtype of a host wire buffer

    @classmethod
    def wire_torch_dtype(cls):
        import torch
        return getattr(torch, cls.WIRE)

    @classmethod
    def wire_like(cls, x):
        """A wire-format buffer of x's kind, device and element count (a
        compressed context's staging buffer)."""
        if _is_torch(x):
            import torch
            return torch.empty(x.numel(), dtype=cls.wire_torch_dtype(), device=x.device)
        return np.empty(x.size, dtype=cls.NUMPY)

    @classmethod
    def _host_wire(cls, x):
        """A CPU torch view, of the wire dtype, of a host wire buffer."""
        return _as_host_tensor(x)

    @classmethod
    def _is_wire(cls, x) -> bool:
        raise NotImplementedError

    @classmethod
    def compresses(cls, tensor) -> bool:
        return _is_floating(tensor) and not cls._is_wire(tensor)

    @classmethod
    def compress(cls, tensor):
        ctx = tensor.dtype
        if not cls.compresses(tensor):
            return tensor, ctx
        import torch
        if _on_device(tensor):
            from . import torch_ops  # noqa: F401  (registers torch.ops.bpsr.*)
            with torch.cuda.device(tensor.device):
                return getattr(torch.ops.bpsr, f"compress_{cls.NAME}")(tensor.contiguous()), ctx
        if _is_torch(tensor):
            return tensor.to(cls.wire_torch_dtype()), ctx
        out = np.empty(tensor.shape, dtype=cls.NUMPY)
        return cls.compress_into(out, np.ascontiguousarray(tensor)), ctx

    @classmethod
    def compress_into(cls, out, tensor):
        """``compress`` into a preallocated wire buffer of the same kind and
        element count (push_pull's staging buffer); returns ``out``."""
        import torch
        if _on_device(tensor):
            from . import torch_ops  # noqa: F401
            with torch.cuda.device(tensor.device):
                getattr(torch.ops.bpsr, f"compress_{cls.NAME}_out")(out.reshape(-1),
                                                                    tensor.reshape(-1))
            return out
        cls._host_wire(out).reshape(-1).copy_(_as_host_tensor(tensor).reshape(-1))
        return out

    @classmethod
    def decompress(cls, tensor, ctx):
        """``ctx``: the dtype ``compress`` returned."""
        if ctx is None or tensor.dtype == ctx:
            return tensor
        if _is_torch(tensor):
            if not ctx.is_floating_point:
                return tensor
            import torch
            out = torch.empty(tensor.shape, dtype=ctx, device=tensor.device)
            return cls.decompress_into(out, tensor.contiguous())
        if not np.issubdtype(ctx, np.floating):
            return tensor
        out = np.empty(tensor.shape, dtype=ctx)
        return cls.decompress_into(out, np.ascontiguousarray(tensor))

    @classmethod
    def decompress_into(cls, out, compressed, divisor: int = 1, stats=None,
                        plans: CastPlanCache | None = None):
        """``out[i] = T(compressed[i])``, or ``T(wire(compressed[i] / divisor))``
        for a divisor above 1 (divide on the 2-byte value, then widen), in one
        pass; returns ``out``.  ``stats``: a float64 tensor or array of shape
        ``(2,)`` — on ``out``'s device for a device tensor — that receives
        ``decompress_stats(out)``; a device tensor then goes through a
        one-segment cast plan (from ``plans`` if given, else built and
        destroyed here, which waits for the launch)."""
        if int(divisor) < 1:
            raise ValueError(f"divisor {divisor} < 1")
        import torch
        if stats is not None:
            _check_stats(stats, (2,))
            if _on_device(out) or _on_device(compressed):
                _cast_many(cls, [(out, compressed)], False, divisor, plans,
                           stats=stats.reshape(1, 2))
                return out
            if _on_device(stats):
                raise ValueError(f"stats is on {stats.device}, the tensor on the host")
            cls.decompress_into(out, compressed, divisor)
            stats[0], stats[1] = decompress_stats(out)
            return out
        if _on_device(out):
            from . import torch_ops  # noqa: F401
            with torch.cuda.device(out.device):
                getattr(torch.ops.bpsr, f"decompress_{cls.NAME}_out")(
                    out.reshape(-1), compressed.reshape(-1), int(divisor))
            return out
        q = cls._host_wire(compressed).reshape(-1)
        if int(divisor) > 1:
            q = q.clone().div_(int(divisor))
        _as_host_tensor(out).reshape(-1).copy_(q)
        return out

    @classmethod
    def compress_many_into(cls, outs, tensors, plans: CastPlanCache | None = None):
        """``compress_into(outs[i], tensors[i])`` for every i, the device
        tensors as one cast-plan launch per (device, dtype); returns ``outs``.
        ``plans`` keeps the plans for the next call over the same tensors;
        without it a plan is built and destroyed here."""
        if len(outs) != len(tensors):
            raise ValueError("compress_many_into: as many outputs as tensors")
        _cast_many(cls, list(zip(tensors, outs)), True, 1, plans)
        return outs

    @classmethod
    def decompress_many_into(cls, outs, compressed, divisor: int = 1,
                             plans: CastPlanCache | None = None, stats=None,
                             clip_norm=None, clip_eps: float = 1e-6, unscale=None):
        """``decompress_into(outs[i], compressed[i], divisor)`` for every i,
        the device tensors as one cast-plan launch per (device, dtype);
        returns ``outs``.  ``stats``: a float64 tensor or array of shape
        ``(len(outs), 2)`` where the outputs live; row i receives
        ``decompress_stats(outs[i])``.

        With ``clip_norm`` the outputs are clipped to that global L2 norm and
        multiplied by ``unscale`` (a number, or a 1-element float32 device
        tensor: GradScaler's inverse scale) inside the decompress: measure,
        ``clip_record(rows, clip_norm, clip_eps, unscale)``, then the decompress
        times the record's ``mult``, one rounding an element.  The record is
        returned (a ``reducer.ClipRecord`` on the outputs' device — they share
        one — or :class:`ClipValues` for host outputs); ``stats`` then
        receives the statistics BEFORE the clip: those of the values a plain
        decompress would have written."""
        if clip_norm is None:
            if unscale is not None:
                raise ValueError("unscale goes with clip_norm")
            return cls.decompress_many_with(outs, compressed, None, divisor, plans, stats)
        return cls._decompress_many_clipped(outs, compressed, None, divisor, plans, stats,
                                            clip_norm, clip_eps, unscale)

    @classmethod
    def _decompress_many_clipped(cls, outs, compressed, extras, divisor, plans, stats, clip_norm,
                                 clip_eps, unscale):
        """measure, clip record, scaled decompress over the same cached plans;
        returns the record."""
        n = len(outs)
        if len(compressed) != n:
            raise ValueError("decompress_many_into: as many outputs as compressed tensors")
        if stats is not None:
            _check_stats(stats, (n, 2))
        if not clip_norm > 0 or not np.isfinite(clip_norm):
            raise ValueError(f"clip_norm {clip_norm} is not a finite positive number")
        if not clip_eps >= 0:
            raise ValueError(f"clip_eps {clip_eps} < 0")
        devices = {o.device if _on_device(o) else None for o in outs}
        if len(devices) > 1:
            raise ValueError("clip_norm: the outputs live in one place, a device or the host")
        if devices in (set(), {None}):
            if _is_torch(unscale) and _on_device(unscale):
                raise ValueError(f"unscale is on {unscale.device}, the outputs on the host")
            rows = stats if stats is not None else np.empty((n, 2), dtype=np.float64)
            cls.measure_many_with(outs, compressed, extras, divisor, plans, rows)
            rec = clip_record(rows, clip_norm, clip_eps,
                              unscale.item() if _is_torch(unscale) else unscale)
            cls.decompress_many_with(outs, compressed, extras, divisor, plans, scale=rec.mult)
            return rec
        import torch
        from .torch_ops import _red
        device = next(iter(devices))
        cache = CastPlanCache(4) if plans is None else plans
        try:
            whole = stats is not None and stats.is_contiguous()
            rows = stats if whole else torch.empty((n, 2), dtype=torch.float64, device=device)
            inv = unscale
            if inv is not None and not _is_torch(inv):
                inv = torch.tensor([float(inv)], dtype=torch.float32, device=device)
            cls.measure_many_with(outs, compressed, extras, divisor, cache, rows)
            if stats is not None and not whole:
                stats.copy_(rows)
            with torch.cuda.device(device):
                rec = _red().clip_record(rows, clip_norm, clip_eps, inv)
            cls.decompress_many_with(outs, compressed, extras, divisor, cache, scale=rec.mult)
        finally:
            if plans is None:
                cache.close()             # waits for the launches
        return rec

    # The forms that take the scheme's per-tensor operand — an error-feedback
    # residual, a stochastic-rounding SrKey, None for the plain cast — as cast
    # plans and push_pull's contexts carry it.  The scheme mix-ins override all
    # but the last; given None, theirs are these.
    @classmethod
    def cast_extra(cls, tensor, key):
        """The operand a context of this compressor keeps for ``tensor``;
        ``key()`` is the context's stochastic-rounding key."""
        return None

    @classmethod
    def _check_segment(cls, half, wide, extra) -> None:
        """The device operands of one cast-plan segment."""
        from .torch_ops import _check_cast
        _check_cast(half, wide, cls.wire_torch_dtype())

    @classmethod
    def compress_with(cls, out, tensor, extra=None, step=None):
        """This compressor's compress of one tensor: ``compress_into``,
        ``compress_ef_into`` or ``compress_sr_into``."""
        return cls.compress_into(out, tensor)

    @classmethod
    def compress_many_with(cls, outs, tensors, extras, step=None,
                           plans: CastPlanCache | None = None):
        """... of many: ``compress_many_into``, ``compress_many_ef_into`` or
        ``compress_many_sr_into``."""
        return cls.compress_many_into(outs, tensors, plans)

    @classmethod
    def decompress_many_with(cls, outs, compressed, extras, divisor: int = 1,
                             plans: CastPlanCache | None = None, stats=None, scale=None):
        """``decompress_many_into``; ``extras`` (those of the compress over the
        same tensors, or None) only name the plan: every scheme's decompress is
        the plain one, so one cached plan serves both directions, and residuals
        are not touched.  ``scale``: every value written is multiplied by it
        (a 1-element float32 device tensor for device outputs, a number for
        host ones), rounded once to the output's dtype; it excludes
        ``stats``."""
        if len(outs) != len(compressed):
            raise ValueError("decompress_many_into: as many outputs as compressed tensors")
        _cast_many(cls, list(zip(outs, compressed)), False, divisor, plans, extras=extras,
                   stats=stats, scale=scale)
        return outs

    @classmethod
    def measure_many_with(cls, outs, compressed, extras, divisor: int = 1,
                          plans: CastPlanCache | None = None, stats=None):
        """The statistics ``decompress_many_with(..., stats=stats)`` would
        report, through the same cached plans, WITHOUT the decompress: nothing
        is written to ``outs`` (device outputs: the 2-byte side alone is read;
        host outputs: the definition on a scratch copy).  Returns ``stats``."""
        if len(outs) != len(compressed):
            raise ValueError("measure_many_with: as many outputs as compressed tensors")
        if stats is None:
            raise ValueError("measure_many_with needs stats")
        _cast_many(cls, list(zip(outs, compressed)), False, divisor, plans, extras=extras,
                   stats=stats, measure=True)
        return stats

    @classmethod
    def _check_sgd_segment(cls, i: int, param, half, mom) -> bool:
        """The operands of one SGD segment; True when they are on a device."""
        dev = [_on_device(x) for x in (param, half, mom)]
        if any(dev) != all(dev):
            raise ValueError(f"apply_sgd: tensor {i}'s parameter, compressed tensor and momentum "
                             f"live in one place, a device or the host")
        if not _is_f32(param) or not _is_f32(mom):
            raise ValueError(f"apply_sgd: tensor {i} needs a float32 parameter and a float32 "
                             f"momentum buffer, got {param.dtype} and {mom.dtype}")
        size = (lambda x: int(x.numel()) if _is_torch(x) else int(x.size))
        for x in (half, mom):
            if size(x) != size(param):
                raise ValueError(f"apply_sgd: tensor {i}'s operands differ in size")
        if dev[0]:
            if half.dtype != cls.wire_torch_dtype():
                raise ValueError(f"apply_sgd: the compressed tensor must be {cls.WIRE}, "
                                 f"got {half.dtype}")
            if not (param.device == half.device == mom.device):
                raise ValueError(f"apply_sgd: tensor {i}'s operands are on different devices")
            if not (param.is_contiguous() and half.is_contiguous() and mom.is_contiguous()):
                raise ValueError(f"apply_sgd: tensor {i} needs contiguous operands")
        else:
            for x in (param, half, mom):
                ok = x.is_contiguous() if _is_torch(x) else x.flags["C_CONTIGUOUS"]
                if not ok:
                    raise ValueError(f"apply_sgd: tensor {i} needs contiguous operands")
            want = cls.wire_torch_dtype() if _is_torch(half) else cls.NUMPY
            if half.dtype != want:
                raise ValueError(f"apply_sgd: the compressed tensor must be {cls.WIRE}, "
                                 f"got {half.dtype}")
        return dev[0]

    @classmethod
    def apply_sgd_many(cls, params, compressed, momenta, divisor: int = 1, *, lr,
                       momentum: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False,
                       record=None, skip_nonfinite: bool = False,
                       plans: CastPlanCache | None = None):
        """The SGD step inside the decompress: ``params[i]`` and
        ``momenta[i]`` (float32) are updated in place from ``compressed[i]``
        under ``prophet_amd.sgd.sgd_step`` — the gradient
        ``decompress_into(_, compressed[i], divisor)`` would write is never
        written.  Device tensors are grouped by device, each group ONE launch
        of an SGD plan (``byteps_reduce_cast_plan_apply_sgd``) on the current
        stream; CPU tensors and numpy arrays go through ``sgd.py``.

        ``record``: a clip record — ``reducer.ClipRecord`` on the tensors'
        device, or :class:`ClipValues` for host tensors — whose ``mult``
        scales the gradient as ``decompress_many_with(scale=)`` does.  With
        ``skip_nonfinite`` a record whose ``nonfinite`` is not 0 leaves every
        byte of ``params`` and ``momenta``: decided on the device for device
        tensors, with no host round trip; the host path reads the record.
        Returns ``params``."""
        from .sgd import check_hyper, sgd_step
        n = len(params)
        if len(compressed) != n or len(momenta) != n:
            raise ValueError("apply_sgd_many: as many compressed tensors and momenta as parameters")
        if int(divisor) < 1:
            raise ValueError(f"divisor {divisor} < 1")
        check_hyper(lr, momentum, weight_decay, nesterov)
        if skip_nonfinite and record is None:
            raise ValueError("skip_nonfinite needs a clip record")
        groups: dict = {}
        host = []
        for i, (p, h, m) in enumerate(zip(params, compressed, momenta)):
            if cls._check_sgd_segment(i, p, h, m):
                groups.setdefault(p.device, []).append((p.reshape(-1), h.reshape(-1),
                                                        m.reshape(-1)))
            else:
                host.append((p, h, m))
        rec_dev = getattr(getattr(record, "tensor", None), "device", None)
        if host:
            mult, skip = None, False
            if record is not None:
                if rec_dev is not None and rec_dev.type == "cuda" and not groups:
                    raise ValueError(f"record is on {rec_dev}, the tensors on the host")
                val = (lambda x: x.item() if _is_torch(x) else x)
                mult = np.float32(val(record.mult))
                skip = bool(skip_nonfinite) and float(val(record.nonfinite)) != 0.0
            for p, h, m in ([] if skip else host):
                pa = (p.detach().numpy() if _is_torch(p) else p).reshape(-1)
                ma = (m.detach().numpy() if _is_torch(m) else m).reshape(-1)
                if _is_torch(h):
                    import torch
                    ha = h.detach().reshape(-1).view(torch.int16).numpy().view(np.uint16)
                else:
                    ha = h.reshape(-1).view(np.uint16)
                pn, mn = sgd_step(pa, ma, ha, cls.NAME, divisor, lr=lr, momentum=momentum,
                                  weight_decay=weight_decay, nesterov=nesterov, mult=mult)
                pa[:], ma[:] = pn, mn
        if not groups:
            return params
        import torch
        from .dtypes import from_torch
        from .reducer import ClipRecord
        if record is not None and not isinstance(record, ClipRecord):
            raise ValueError("apply_sgd_many: device tensors take a reducer.ClipRecord")
        wire = from_torch(cls.wire_torch_dtype())
        for device, segs in groups.items():
            if record is not None and record.tensor.device != device:
                raise ValueError(f"record is on {record.tensor.device}, tensors on {device}")
            with torch.cuda.device(device):
                plan = plans.get_sgd(segs, wire) if plans is not None \
                    else _new_sgd_plan(segs, wire)
                try:
                    plan.apply(int(divisor), lr=lr, momentum=momentum,
                               weight_decay=weight_decay, nesterov=nesterov, record=record,
                               skip_nonfinite=skip_nonfinite,
                               stream=torch.cuda.current_stream(device))
                finally:
                    if plans is None:
                        plan.close()      # waits for the launch
        return params

    @classmethod
    def apply_sgd_into(cls, param, compressed, momentum_buf, divisor: int = 1, *, lr,
                       momentum: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False,
                       record=None, skip_nonfinite: bool = False,
                       plans: CastPlanCache | None = None):
        """``apply_sgd_many`` of one tensor: a device tensor goes through a
        one-segment SGD plan (from ``plans`` if given, else built and destroyed
        here, which waits for the launch), as ``decompress_into(stats=)``
        does.  Returns ``param``."""
        cls.apply_sgd_many([param], [compressed], [momentum_buf], divisor, lr=lr,
                           momentum=momentum, weight_decay=weight_decay, nesterov=nesterov,
                           record=record, skip_nonfinite=skip_nonfinite, plans=plans)
        return param


class FP16Compressor(_CastCompressor):
    """Floating tensors travel as fp16."""

    WIRE_DTYPE, WIRE, NAME, NUMPY = 2, "float16", "fp16", np.float16    # DType.FLOAT16

    @classmethod
    def _is_wire(cls, x) -> bool:
        return _is_half(x)


class BF16Compressor(_CastCompressor):
    """Floating tensors travel as bf16 (f32's exponent range: a sum that fp16
    turns into inf stays finite).  A numpy wire buffer holds raw uint16 bits,
    so for numpy ``decompress`` goes by ``ctx`` alone."""

    WIRE_DTYPE, WIRE, NAME, NUMPY = 11, "bfloat16", "bf16", np.uint16   # DType.BFLOAT16

    @classmethod
    def _is_wire(cls, x) -> bool:
        return _is_bf16(x)

    @classmethod
    def _host_wire(cls, x):
        return _as_host_bf16(x)


def _is_f32(x) -> bool:
    if _is_torch(x):
        import torch
        return x.dtype == torch.float32
    return x.dtype == np.float32


def _mx_dtype(x):
    """The DType id of a tensor the block-scaled wires take — float32, float16
    or (torch) bfloat16 — else ``None``."""
    return 0 if _is_f32(x) else 2 if _is_half(x) else 11 if _is_bf16(x) else None


_MX_OUT = {0: None, 2: "float16", 11: "bfloat16"}     # DType id: mx.narrow's out_dtype


def _mx_host(x):
    """A host tensor of a block-scaled wire as the definition takes it: a flat
    numpy view, a bf16 tensor as its uint16 bits."""
    if _is_bf16(x):
        import torch
        return x.detach().view(torch.int16).numpy().view(np.uint16).reshape(-1)
    return (x.detach().numpy() if _is_torch(x) else x).reshape(-1)


def _run_by_dtype(groups, plans, get, launch) -> None:
    """``OneBitEFCompressor._run`` over segments grouped by ``(device,
    dtype)``: one plan, ``get(cache, segs, dtype)``, and one launch a group."""
    for (device, dt), segs in groups.items():
        OneBitEFCompressor._run({device: segs}, plans,
                                lambda cache, s, dt=dt: get(cache, s, dt), launch)


class _ErrorFeedback:
    """Error feedback over a cast compressor (mixed in ahead of it): a
    per-tensor f32 residual takes what the wire format could not carry and
    gives it back before the next cast.  float32 tensors only — everything
    else, f64 and the 2-byte floats included, passes through uncompressed.
    ``compress(tensor)`` is inherited and stays the plain, stateless cast (no
    residual to read or write); ``decompress*`` is inherited unchanged."""

    ERROR_FEEDBACK = True

    @classmethod
    def compresses(cls, tensor) -> bool:
        return _is_f32(tensor)

    @classmethod
    def cast_extra(cls, tensor, key):
        return cls.residual_like(tensor)

    @classmethod
    def _check_segment(cls, half, wide, resid) -> None:
        if resid is None:
            return super()._check_segment(half, wide, None)
        from .torch_ops import _check_cast_ef
        _check_cast_ef(half, resid, wide, cls.wire_torch_dtype())

    @classmethod
    def compress_with(cls, out, tensor, resid=None, step=None):
        return cls.compress_into(out, tensor) if resid is None else \
            cls.compress_ef_into(out, resid, tensor)

    @classmethod
    def compress_many_with(cls, outs, tensors, residuals, step=None,
                           plans: CastPlanCache | None = None):
        return cls.compress_many_ef_into(outs, residuals, tensors, plans)

    @classmethod
    def residual_like(cls, x):
        """A zeroed f32 residual of x's kind, device and element count."""
        if _is_torch(x):
            import torch
            return torch.zeros(x.numel(), dtype=torch.float32, device=x.device)
        return np.zeros(x.size, dtype=np.float32)

    @classmethod
    def compress_ef_into(cls, out, residual, tensor):
        """``c = tensor + residual``; ``out = wire(c)``; ``residual = c -
        out.float()`` where that is finite, +0.0 elsewhere — in place, one
        pass on the device; returns ``out``."""
        import torch
        if not cls.compresses(tensor) or not _is_f32(residual):
            raise ValueError("error feedback needs a float32 tensor and a float32 residual")
        if _on_device(tensor):
            from . import torch_ops  # noqa: F401
            with torch.cuda.device(tensor.device):
                getattr(torch.ops.bpsr, f"compress_{cls.NAME}_ef_out")(
                    out.reshape(-1), residual.reshape(-1), tensor.reshape(-1))
            return out
        g = _as_host_tensor(tensor).reshape(-1)
        r = _as_host_tensor(residual).reshape(-1)
        if r.numel() != g.numel():
            raise ValueError("error feedback: residual and tensor differ in size")
        c = g + r
        w = c.to(cls.wire_torch_dtype())
        b = w.to(torch.float32)
        r.copy_(torch.where(torch.isfinite(b), c - b, torch.zeros_like(c)))
        cls._host_wire(out).reshape(-1).copy_(w)
        return out

    @classmethod
    def compress_many_ef_into(cls, outs, residuals, tensors, plans: CastPlanCache | None = None):
        """``compress_ef_into(outs[i], residuals[i], tensors[i])`` for every
        i, the device tensors as one error-feedback cast-plan launch per
        device; returns ``outs``."""
        if len(outs) != len(tensors) or len(residuals) != len(tensors):
            raise ValueError("compress_many_ef_into: as many outputs and residuals as tensors")
        for t, r in zip(tensors, residuals):
            if not cls.compresses(t) or not _is_f32(r):
                raise ValueError("error feedback needs float32 tensors and float32 residuals")
        _cast_many(cls, list(zip(tensors, outs)), True, 1, plans, extras=list(residuals))
        return outs

    @classmethod
    def decompress_many_into(cls, outs, compressed, divisor: int = 1,
                             plans: CastPlanCache | None = None, residuals=None, stats=None,
                             clip_norm=None, clip_eps: float = 1e-6, unscale=None):
        """The inherited decompress, ``stats`` and ``clip_norm`` included.  ``residuals`` (those given to
        ``compress_many_ef_into`` over the same tensors) only names the plan:
        the error-feedback plan's own decompress is the plain one, so one
        cached plan serves both directions; the residuals are not touched."""
        extras = None if residuals is None else list(residuals)
        if clip_norm is None:
            if unscale is not None:
                raise ValueError("unscale goes with clip_norm")
            return cls.decompress_many_with(outs, compressed, extras, divisor, plans, stats)
        return cls._decompress_many_clipped(outs, compressed, extras, divisor, plans, stats,
                                            clip_norm, clip_eps, unscale)


class FP16EFCompressor(_ErrorFeedback, FP16Compressor):
    """float32 tensors travel as fp16 with error feedback."""


class BF16EFCompressor(_ErrorFeedback, BF16Compressor):
    """float32 tensors travel as bf16 with error feedback."""


def _sr_keys(keys) -> list:
    """Keys (mod 2^32) as a stochastic-rounding plan's segments carry them."""
    return [SrKey(int(k) & 0xffffffff) for k in keys]


class _StochasticRounding:
    """Stochastic rounding over a cast compressor (mixed in ahead of it):
    round up with a probability equal to the dropped fraction, under bits
    that are a pure function of ``(key, step, element index)``
    (``prophet_amd/sr.py``).  float32 tensors only — everything else passes
    through uncompressed.  ``compress(tensor)`` is inherited and stays the
    plain, deterministic cast (it has no key or step); ``decompress*`` is
    inherited unchanged."""

    STOCHASTIC = True

    @classmethod
    def compresses(cls, tensor) -> bool:
        return _is_f32(tensor)

    @classmethod
    def cast_extra(cls, tensor, key):
        return SrKey(key())

    @classmethod
    def _check_segment(cls, half, wide, key) -> None:
        if key is None:
            return super()._check_segment(half, wide, None)
        from .torch_ops import _check_cast_sr
        _check_cast_sr(half, wide, cls.wire_torch_dtype())

    @classmethod
    def compress_with(cls, out, tensor, key=None, step=None):
        return cls.compress_into(out, tensor) if key is None else \
            cls.compress_sr_into(out, tensor, key, step)

    @classmethod
    def compress_many_with(cls, outs, tensors, keys, step=None,
                           plans: CastPlanCache | None = None):
        return cls.compress_many_sr_into(outs, tensors, keys, step, plans)

    @classmethod
    def compress_sr_into(cls, out, tensor, key: int, step: int):
        """``out = sr(tensor; key, step)``: element ``i`` rounded under 16
        bits of Philox2x32-10(``i >> 2``, ``step``, ``key``); one pass on the
        device; returns ``out``."""
        if not cls.compresses(tensor):
            raise ValueError("stochastic rounding needs a float32 tensor")
        if _on_device(tensor):
            import torch
            from . import torch_ops  # noqa: F401
            with torch.cuda.device(tensor.device):
                getattr(torch.ops.bpsr, f"compress_{cls.NAME}_sr_out")(
                    out.reshape(-1), tensor.reshape(-1), int(key) & 0xffffffff,
                    int(step) & 0xffffffff)
            return out
        from .sr import sr_round
        g = tensor.detach().numpy() if _is_torch(tensor) else tensor
        if _is_torch(out):
            import torch
            if out.dtype != cls.wire_torch_dtype():
                raise ValueError(f"the compressed tensor must be {cls.WIRE}, got {out.dtype}")
            o = out.reshape(-1).view(torch.int16).numpy().view(np.uint16)
        else:
            o = out.reshape(-1).view(np.uint16)
        if o.size != g.size:
            raise ValueError("stochastic rounding: output and tensor differ in size")
        o[:] = sr_round(g, key, step, cls.NAME)
        return out

    @classmethod
    def compress_many_sr_into(cls, outs, tensors, keys, step: int,
                              plans: CastPlanCache | None = None):
        """``compress_sr_into(outs[i], tensors[i], keys[i], step)`` for every
        i, the device tensors as one stochastic-rounding cast-plan launch per
        device; returns ``outs``."""
        if len(outs) != len(tensors) or len(keys) != len(tensors):
            raise ValueError("compress_many_sr_into: as many outputs and keys as tensors")
        for t in tensors:
            if not cls.compresses(t):
                raise ValueError("stochastic rounding needs float32 tensors")
        _cast_many(cls, list(zip(tensors, outs)), True, 1, plans, extras=_sr_keys(keys), step=step)
        return outs

    @classmethod
    def decompress_many_into(cls, outs, compressed, divisor: int = 1,
                             plans: CastPlanCache | None = None, keys=None, stats=None,
                             clip_norm=None, clip_eps: float = 1e-6, unscale=None):
        """The inherited decompress, ``stats`` and ``clip_norm`` included.  ``keys`` (those given to
        ``compress_many_sr_into`` over the same tensors) only names the plan:
        the stochastic-rounding plan's own decompress is the plain one, so one
        cached plan serves both directions."""
        extras = None if keys is None else _sr_keys(keys)
        if clip_norm is None:
            if unscale is not None:
                raise ValueError("unscale goes with clip_norm")
            return cls.decompress_many_with(outs, compressed, extras, divisor, plans, stats)
        return cls._decompress_many_clipped(outs, compressed, extras, divisor, plans, stats,
                                            clip_norm, clip_eps, unscale)


class FP16SRCompressor(_StochasticRounding, FP16Compressor):
    """float32 tensors travel as fp16, stochastically rounded."""


class BF16SRCompressor(_StochasticRounding, BF16Compressor):
    """float32 tensors travel as bf16, stochastically rounded."""


def _payload_array(x):
    """A host payload (uint8 CPU tensor or numpy array) as a flat numpy view."""
    a = x.detach().numpy() if _is_torch(x) else x
    if a.dtype != np.uint8:
        raise ValueError(f"a payload is uint8, got {a.dtype}")
    return a.reshape(-1)


class OneBitEFCompressor(Compressor):
    """float32 tensors travel as one bit an element plus one float32 scale,
    with error feedback (``prophet_amd/onebit.py`` is the definition): 32x
    smaller than float32.  A payload is a flat uint8 buffer of
    ``onebit.payload_bytes(n)`` bytes, on the device 16-byte aligned.  Device
    tensors go through 1-bit plans (``byteps_reduce_onebit_*``,
    ``prophet_amd/csrc/bpsr_k_onebit.hip``): a compress of many tensors is
    three launches per device, a fold of many is one; CPU tensors and numpy
    arrays go through ``onebit.py``.  Everything but float32 passes through.

    A payload is no element-wise dtype, so the PS server cannot fold it:
    ``Worker.init_tensor`` takes this compressor only over a frontend that
    carries packed payloads (``ServerFrontend``: ``packed_round.PackedRound``
    runs ``refold_many_into``, the two-way round of DESIGN.md §11.11).
    ``fold_many_into`` is what a worker that gathered every worker's payload
    computes."""

    ERROR_FEEDBACK = True
    PACKED = True
    SERVER_ROUND = True

    @classmethod
    def compresses(cls, tensor) -> bool:
        return _is_f32(tensor)

    @classmethod
    def payload_like(cls, x):
        """An uninitialised payload buffer for x, of x's kind and device."""
        from .onebit import payload_bytes
        n = int(x.numel()) if _is_torch(x) else int(x.size)
        if _is_torch(x):
            import torch
            return torch.empty(payload_bytes(n), dtype=torch.uint8, device=x.device)
        return np.empty(payload_bytes(n), dtype=np.uint8)

    @classmethod
    def payload_nbytes(cls, n: int) -> int:
        """The bytes of the payload of ``n`` elements."""
        from .onebit import payload_bytes
        return payload_bytes(n)

    @classmethod
    def init_payload(cls, n: int):
        """The payload of ``n`` zeros, a new uint8 array: the header ``{0.0,
        n}`` and zeros — what a key's init push carries."""
        zero = np.zeros(cls.payload_nbytes(n), dtype=np.uint8)
        zero[4:12] = np.array([int(n)], dtype="<u8").view(np.uint8)
        return zero

    residual_like = classmethod(_ErrorFeedback.residual_like.__func__)

    @classmethod
    def compress(cls, tensor):
        """The stateless form: one step from a zero residual, which is
        dropped.  ``ctx`` is ``(dtype, shape)``."""
        ctx = (tensor.dtype, tuple(tensor.shape))
        if not cls.compresses(tensor):
            return tensor, ctx
        flat = tensor.contiguous() if _is_torch(tensor) else np.ascontiguousarray(tensor)
        return cls.compress_ef_into(cls.payload_like(flat), cls.residual_like(flat), flat), ctx

    @classmethod
    def decompress(cls, payload, ctx):
        dtype, shape = ctx
        if payload.dtype == dtype:
            return payload
        if _is_torch(payload):
            import torch
            out = torch.empty(shape, dtype=dtype, device=payload.device)
        else:
            out = np.empty(shape, dtype=dtype)
        return cls.decompress_into(out, payload)

    @classmethod
    def compress_ef_into(cls, payload, residual, tensor, plans: CastPlanCache | None = None):
        """``payload, residual = onebit.compress(tensor, residual)``, the
        residual in place; returns ``payload``."""
        cls.compress_many_ef_into([payload], [residual], [tensor], plans)
        return payload

    @classmethod
    def compress_many_ef_into(cls, payloads, residuals, tensors,
                              plans: CastPlanCache | None = None):
        """``compress_ef_into`` for every i, the device tensors as one 1-bit
        plan per device (three launches); returns ``payloads``."""
        from . import onebit
        if len(payloads) != len(tensors) or len(residuals) != len(tensors):
            raise ValueError("compress_many_ef_into: as many payloads and residuals as tensors")
        groups: dict = {}
        for i, (p, r, t) in enumerate(zip(payloads, residuals, tensors)):
            if not cls.compresses(t) or not _is_f32(r):
                raise ValueError("onebit_ef needs float32 tensors and float32 residuals")
            dev = [_on_device(x) for x in (p, r, t)]
            if any(dev) != all(dev):
                raise ValueError(f"onebit_ef: tensor {i}'s operands live in one place, a device "
                                 f"or the host")
            if dev[0]:
                cls._check_device_segment(i, t, r, payload=p)
                groups.setdefault(t.device, []).append((t.reshape(-1), r.reshape(-1), p))
                continue
            ra = (r.detach().numpy() if _is_torch(r) else r).reshape(-1)
            ga = t.detach().numpy() if _is_torch(t) else t
            pa = _payload_array(p)
            if ra.size != ga.size or pa.size != onebit.payload_bytes(ga.size):
                raise ValueError(f"onebit_ef: tensor {i}'s operands differ in size")
            pa[:], ra[:] = onebit.compress(ga, ra)
        cls._run(groups, plans, lambda cache, segs: cache.get_onebit(segs),
                 lambda plan, stream: plan.compress(stream=stream))
        return payloads

    @classmethod
    def decompress_into(cls, out, payload, divisor: int = 1, plans: CastPlanCache | None = None):
        """``out = onebit.decode(payload)`` (divided by ``divisor`` above 1):
        the one-source fold; returns ``out``."""
        cls.fold_many_into([out], [[payload]], divisor, plans)
        return out

    @classmethod
    def fold_many_into(cls, outs, payload_lists, divisor: int = 1,
                       plans: CastPlanCache | None = None):
        """``outs[i] = onebit.fold(payload_lists[i], outs[i].size, divisor)``
        for every i — every list of the same length N, 1..16 — the device
        tensors as one 1-bit fold plan per device (ONE launch); returns
        ``outs``."""
        from . import onebit
        if len(outs) != len(payload_lists):
            raise ValueError("fold_many_into: as many payload lists as outputs")
        if int(divisor) < 1:
            raise ValueError(f"divisor {divisor} < 1")
        nsrc = len(payload_lists[0]) if payload_lists else 1
        if not 1 <= nsrc <= onebit.MAX_SRCS or any(len(ps) != nsrc for ps in payload_lists):
            raise ValueError(f"fold_many_into: every output takes the same 1..{onebit.MAX_SRCS} "
                             f"payloads")
        groups: dict = {}
        for i, (o, ps) in enumerate(zip(outs, payload_lists)):
            if not _is_f32(o):
                raise ValueError(f"onebit_ef: output {i} must be float32, got {o.dtype}")
            dev = [_on_device(x) for x in [o] + list(ps)]
            if any(dev) != all(dev):
                raise ValueError(f"onebit_ef: output {i} and its payloads live in one place, a "
                                 f"device or the host")
            if dev[0]:
                for p in ps:
                    cls._check_device_segment(i, o, payload=p)
                groups.setdefault(o.device, []).append((o.reshape(-1), list(ps)))
                continue
            oa = (o.detach().numpy() if _is_torch(o) else o).reshape(-1)
            oa[:] = onebit.fold([_payload_array(p) for p in ps], oa.size, divisor)
        cls._run(groups, plans, lambda cache, segs: cache.get_onebit_fold(segs, nsrc),
                 lambda plan, stream: plan.launch(int(divisor), stream=stream))
        return outs

    @classmethod
    def refold_many_into(cls, out_payloads, residuals, payload_lists,
                         plans: CastPlanCache | None = None):
        """The server round: ``out_payloads[i], residuals[i] =
        onebit.refold(payload_lists[i], residuals[i].size, residuals[i])`` for
        every i — every list of the same length N, 1..16, the residual in
        place — the device tensors as one 1-bit refold plan per device (three
        launches, the folded sum never written); returns ``out_payloads``."""
        from . import onebit
        if len(out_payloads) != len(payload_lists) or len(residuals) != len(payload_lists):
            raise ValueError("refold_many_into: as many output payloads and residuals as "
                             "payload lists")
        nsrc = len(payload_lists[0]) if payload_lists else 1
        if not 1 <= nsrc <= onebit.MAX_SRCS or any(len(ps) != nsrc for ps in payload_lists):
            raise ValueError(f"refold_many_into: every segment takes the same "
                             f"1..{onebit.MAX_SRCS} payloads")
        groups: dict = {}
        for i, (o, r, ps) in enumerate(zip(out_payloads, residuals, payload_lists)):
            if not _is_f32(r):
                raise ValueError(f"onebit_ef: residual {i} must be float32, got {r.dtype}")
            dev = [_on_device(x) for x in [o, r] + list(ps)]
            if any(dev) != all(dev):
                raise ValueError(f"onebit_ef: segment {i}'s operands live in one place, a device "
                                 f"or the host")
            if dev[0]:
                for p in [o] + list(ps):
                    cls._check_device_segment(i, r, payload=p)
                groups.setdefault(r.device, []).append((list(ps), r.reshape(-1), o))
                continue
            ra = (r.detach().numpy() if _is_torch(r) else r).reshape(-1)
            oa = _payload_array(o)
            if oa.size != onebit.payload_bytes(ra.size):
                raise ValueError(f"onebit_ef: segment {i}'s operands differ in size")
            oa[:], ra[:] = onebit.refold([_payload_array(p) for p in ps], ra.size, ra)
        cls._run(groups, plans, lambda cache, segs: cache.get_onebit_refold(segs, nsrc),
                 lambda plan, stream: plan.launch(stream=stream))
        return out_payloads

    @staticmethod
    def _check_device_segment(i: int, tensor, resid=None, payload=None) -> None:
        """One device segment: contiguous float32 operands of one size and a
        flat uint8 payload of the payload's size, all on one device."""
        import torch
        from .onebit import payload_bytes
        for x in (tensor, resid):
            if x is not None and (not x.is_contiguous() or x.device != tensor.device
                                  or x.numel() != tensor.numel()):
                raise ValueError(f"onebit_ef: tensor {i} needs contiguous operands of one size "
                                 f"on one device")
        if payload.dtype != torch.uint8 or not payload.is_contiguous() or payload.dim() != 1 \
                or payload.device != tensor.device \
                or payload.numel() != payload_bytes(tensor.numel()):
            raise ValueError(f"onebit_ef: tensor {i}'s payload must be a flat uint8 tensor of "
                             f"{payload_bytes(tensor.numel())} bytes on {tensor.device}")

    @staticmethod
    def _run(groups, plans, get, launch) -> None:
        """Per device: the plan (from ``plans``, else built and destroyed here,
        which waits for the launch) and its launch on the current stream."""
        if not groups:
            return
        import torch
        for device, segs in groups.items():
            with torch.cuda.device(device):
                cache = plans if plans is not None else CastPlanCache(1)
                try:
                    launch(get(cache, segs), torch.cuda.current_stream(device))
                finally:
                    if plans is None:
                        cache.close()


class TopKEFCompressor(Compressor):
    """float32 tensors travel as their ``k`` values of largest magnitude with
    their indices, with error feedback (``prophet_amd/topk.py`` is the
    definition): ``16 + 8 k`` bytes for ``4 n``.  A payload is
    a flat uint8 buffer (``payload_like(tensor, ratio)``), on the device 16-byte
    aligned, and carries its ``k`` in its size.  Device tensors go through
    top-k plans (``byteps_reduce_topk_*``, ``prophet_amd/csrc/bpsr_k_topk.hip``):
    a compress of many tensors is one fixed sequence of launches per device, a
    fold of many is one launch; CPU tensors and numpy arrays go through
    ``topk.py``, byte for byte the same.  Everything but float32 passes
    through.

    The server round is opt-in and needs a ratio: a key's
    payload size follows from ``n`` and the ratio, so ``Worker.init_tensor``
    takes ``TopKEFCompressor.at(ratio)`` — a cached subclass carrying
    ``RATIO``, with ``payload_nbytes`` and ``init_payload`` — over a
    ``ServerFrontend`` that names that same class in ``packed_wires``; its
    ``packed_round.PackedRound`` store then runs ``refold_many_into`` (the
    compress's launches with the fold fused into the first pass).  This class
    itself, which has no ratio, is refused over every front end.
    ``fold_many_into`` is what a worker that gathered every worker's payload
    computes."""

    ERROR_FEEDBACK = True
    PACKED = True
    RATIO = None                          # set by at(ratio)
    _AT: dict = {}                        # ratio -> its subclass

    @classmethod
    def at(cls, ratio: float):
        """The subclass of this compressor at ``ratio``, the same object for
        the same ratio (so ``in packed_wires`` and grouping by compressor
        work)."""
        ratio = float(ratio)
        if not 0 < ratio <= 1:
            raise ValueError(f"topk_ef: ratio {ratio} outside (0, 1]")
        sub = TopKEFCompressor._AT.get(ratio)
        if sub is None:
            sub = TopKEFCompressor._AT[ratio] = type(
                f"TopKEFCompressor_{ratio!r}", (TopKEFCompressor,), {"RATIO": ratio})
        return sub

    @classmethod
    def payload_nbytes(cls, n: int) -> int:
        """The bytes of the payload of ``n`` elements at ``RATIO``."""
        from .topk import k_for, payload_bytes
        if cls.RATIO is None:
            raise ValueError("topk_ef: a payload's size needs a ratio (TopKEFCompressor.at)")
        return payload_bytes(k_for(n, cls.RATIO) if int(n) else 0)

    @classmethod
    def init_payload(cls, n: int):
        """What a key's init push carries: ``topk.init_payload`` at ``k =
        k_for(n, RATIO)``."""
        from . import topk
        return topk.init_payload(n, (cls.payload_nbytes(n) - topk.HEADER_BYTES) // 8)

    @classmethod
    def compresses(cls, tensor) -> bool:
        return _is_f32(tensor)

    @classmethod
    def payload_like(cls, x, ratio: float | None = None):
        """An uninitialised payload buffer for x at ``k = topk.k_for(n,
        ratio)`` (``RATIO``, else 0.01, unless named), of x's kind and
        device."""
        from .topk import k_for, payload_bytes
        n = int(x.numel()) if _is_torch(x) else int(x.size)
        ratio = (cls.RATIO or 0.01) if ratio is None else ratio
        size = payload_bytes(k_for(n, ratio) if n else 0)
        if _is_torch(x):
            import torch
            return torch.empty(size, dtype=torch.uint8, device=x.device)
        return np.empty(size, dtype=np.uint8)

    residual_like = classmethod(_ErrorFeedback.residual_like.__func__)

    @classmethod
    def compress(cls, tensor, ratio: float | None = None):
        """The stateless form: one step from a zero residual, which is
        dropped.  ``ctx`` is ``(dtype, shape)``."""
        ctx = (tensor.dtype, tuple(tensor.shape))
        if not cls.compresses(tensor):
            return tensor, ctx
        flat = tensor.contiguous() if _is_torch(tensor) else np.ascontiguousarray(tensor)
        return cls.compress_ef_into(cls.payload_like(flat, ratio), cls.residual_like(flat),
                                    flat), ctx

    decompress = classmethod(OneBitEFCompressor.decompress.__func__)

    @classmethod
    def compress_ef_into(cls, payload, residual, tensor, plans: CastPlanCache | None = None):
        """``payload, residual = topk.compress(tensor, residual,
        topk.k_of(payload))``, the residual in place; returns ``payload``."""
        cls.compress_many_ef_into([payload], [residual], [tensor], plans)
        return payload

    @classmethod
    def compress_many_ef_into(cls, payloads, residuals, tensors,
                              plans: CastPlanCache | None = None):
        """``compress_ef_into`` for every i, the device tensors as one top-k
        plan per device; returns ``payloads``."""
        from . import topk
        if len(payloads) != len(tensors) or len(residuals) != len(tensors):
            raise ValueError("compress_many_ef_into: as many payloads and residuals as tensors")
        groups: dict = {}
        for i, (p, r, t) in enumerate(zip(payloads, residuals, tensors)):
            if not cls.compresses(t) or not _is_f32(r):
                raise ValueError("topk_ef needs float32 tensors and float32 residuals")
            dev = [_on_device(x) for x in (p, r, t)]
            if any(dev) != all(dev):
                raise ValueError(f"topk_ef: tensor {i}'s operands live in one place, a device "
                                 f"or the host")
            if dev[0]:
                cls._check_device_segment(i, t, r, payload=p)
                groups.setdefault(t.device, []).append((t.reshape(-1), r.reshape(-1), p))
                continue
            ra = (r.detach().numpy() if _is_torch(r) else r).reshape(-1)
            ga = t.detach().numpy() if _is_torch(t) else t
            pa = _payload_array(p)
            if ra.size != ga.size:
                raise ValueError(f"topk_ef: tensor {i}'s operands differ in size")
            pa[:], ra[:] = topk.compress(ga, ra, topk.k_of(pa))
        OneBitEFCompressor._run(groups, plans, lambda cache, segs: cache.get_topk(segs),
                                lambda plan, stream: plan.compress(stream=stream))
        return payloads

    @classmethod
    def decompress_into(cls, out, payload, divisor: int = 1, plans: CastPlanCache | None = None):
        """The one-source fold (``topk.fold([payload], n, divisor)``); returns
        ``out``."""
        cls.fold_many_into([out], [[payload]], divisor, plans)
        return out

    @classmethod
    def fold_many_into(cls, outs, payload_lists, divisor: int = 1,
                       plans: CastPlanCache | None = None):
        """``outs[i] = topk.fold(payload_lists[i], outs[i].size, divisor)`` for
        every i — every list of the same length N, 1..16, an output's payloads
        of one size — the device tensors as one top-k fold plan per device (ONE
        launch); returns ``outs``."""
        from . import topk
        if len(outs) != len(payload_lists):
            raise ValueError("fold_many_into: as many payload lists as outputs")
        if int(divisor) < 1:
            raise ValueError(f"divisor {divisor} < 1")
        nsrc = len(payload_lists[0]) if payload_lists else 1
        if not 1 <= nsrc <= topk.MAX_SRCS or any(len(ps) != nsrc for ps in payload_lists):
            raise ValueError(f"fold_many_into: every output takes the same 1..{topk.MAX_SRCS} "
                             f"payloads")
        groups: dict = {}
        for i, (o, ps) in enumerate(zip(outs, payload_lists)):
            if not _is_f32(o):
                raise ValueError(f"topk_ef: output {i} must be float32, got {o.dtype}")
            dev = [_on_device(x) for x in [o] + list(ps)]
            if any(dev) != all(dev):
                raise ValueError(f"topk_ef: output {i} and its payloads live in one place, a "
                                 f"device or the host")
            if len({topk.k_of(p) for p in ps}) != 1:
                raise ValueError(f"topk_ef: output {i}'s payloads differ in size")
            if dev[0]:
                for p in ps:
                    cls._check_device_segment(i, o, payload=p)
                groups.setdefault(o.device, []).append((o.reshape(-1), list(ps)))
                continue
            oa = (o.detach().numpy() if _is_torch(o) else o).reshape(-1)
            oa[:] = topk.fold([_payload_array(p) for p in ps], oa.size, divisor)
        OneBitEFCompressor._run(groups, plans, lambda cache, segs: cache.get_topk_fold(segs, nsrc),
                                lambda plan, stream: plan.launch(int(divisor), stream=stream))
        return outs

    @classmethod
    def refold_many_into(cls, out_payloads, residuals, payload_lists,
                         plans: CastPlanCache | None = None):
        """The server round: ``out_payloads[i], residuals[i] =
        topk.refold(payload_lists[i], residuals[i].size, residuals[i], k)`` for
        every i — every list of the same length N, 1..16, ``k`` the payloads'
        size (a segment's sources and output of one size), the float32
        residual in place — the device tensors as one top-k refold plan per
        device (the compress's launches, the folded sum never written);
        returns ``out_payloads``."""
        from . import topk
        if len(out_payloads) != len(payload_lists) or len(residuals) != len(payload_lists):
            raise ValueError("refold_many_into: as many output payloads and residuals as "
                             "payload lists")
        nsrc = len(payload_lists[0]) if payload_lists else 1
        if not 1 <= nsrc <= topk.MAX_SRCS or any(len(ps) != nsrc for ps in payload_lists):
            raise ValueError(f"refold_many_into: every segment takes the same "
                             f"1..{topk.MAX_SRCS} payloads")
        groups: dict = {}
        for i, (o, r, ps) in enumerate(zip(out_payloads, residuals, payload_lists)):
            if not _is_f32(r):
                raise ValueError(f"topk_ef: residual {i} must be float32, got {r.dtype}")
            dev = [_on_device(x) for x in [o, r] + list(ps)]
            if any(dev) != all(dev):
                raise ValueError(f"topk_ef: segment {i}'s operands live in one place, a device "
                                 f"or the host")
            if len({topk.k_of(p) for p in [o] + list(ps)}) != 1:
                raise ValueError(f"topk_ef: segment {i}'s payloads differ in size")
            if dev[0]:
                for p in [o] + list(ps):
                    cls._check_device_segment(i, r, payload=p)
                groups.setdefault(r.device, []).append((list(ps), r.reshape(-1), o))
                continue
            ra = (r.detach().numpy() if _is_torch(r) else r).reshape(-1)
            oa = _payload_array(o)
            oa[:], ra[:] = topk.refold([_payload_array(p) for p in ps], ra.size, ra,
                                       topk.k_of(oa))
        OneBitEFCompressor._run(groups, plans,
                                lambda cache, segs: cache.get_topk_refold(segs, nsrc),
                                lambda plan, stream: plan.launch(stream=stream))
        return out_payloads

    @staticmethod
    def _check_device_segment(i: int, tensor, resid=None, payload=None) -> None:
        """One device segment: contiguous float32 operands of one size and a
        flat uint8 payload of ``k`` entries, ``k`` in ``1..n``, all on one
        device."""
        import torch
        from .topk import k_of
        for x in (tensor, resid):
            if x is not None and (not x.is_contiguous() or x.device != tensor.device
                                  or x.numel() != tensor.numel()):
                raise ValueError(f"topk_ef: tensor {i} needs contiguous operands of one size "
                                 f"on one device")
        n = int(tensor.numel())
        if payload.dtype != torch.uint8 or not payload.is_contiguous() or payload.dim() != 1 \
                or payload.device != tensor.device \
                or not (1 <= k_of(payload) <= n or k_of(payload) == n == 0):
            raise ValueError(f"topk_ef: tensor {i}'s payload must be a flat uint8 tensor of "
                             f"16 + 8 k bytes, k in 1..{n}, on {tensor.device}")


class MXFP8EFCompressor(Compressor):
    """float32 tensors travel in blocks of 32 elements, one power-of-two scale
    byte and 32 OCP e4m3 codes each, with error feedback (``prophet_amd/mx.py``
    is the definition): 8.25 bits an element.
    ``MXFP4EFCompressor`` is the same body over OCP e2m1 codes, 4.25 bits.  A
    payload is a flat uint8 buffer (``payload_like``), on the device 16-byte
    aligned.  Device tensors go through block-scaled plans
    (``byteps_reduce_mx_*``, ``prophet_amd/csrc/bpsr_k_mx.hip``): a compress of
    many tensors is ONE launch per device, and so is a fold of many; CPU
    tensors and numpy arrays go through ``mx.py``, byte for byte the same.
    float16 and bfloat16 tensors are compressed too, from their exact float32
    upcast (the same payload; ``prophet_amd/csrc/bpsr_k_mx_half.hip``, DESIGN.md
    §11.16): the residual stays float32, and a fold writes float32, float16 or
    bfloat16 outputs, converting its float32 result once.  Everything else
    passes through.

    The server round is opt-in: ``Worker.init_tensor`` takes
    these wires, float32 tensors only, over a ``ServerFrontend`` that names
    them in ``packed_wires`` — its ``packed_round.PackedRound`` store then runs
    ``refold_many_into``, one fused launch a round — and refuses them over
    every other front end.  ``fold_many_into`` is what a worker that gathered
    every worker's payload computes."""

    ERROR_FEEDBACK = True
    PACKED = True
    FMT = "fp8"

    @classmethod
    def compresses(cls, tensor) -> bool:
        return _mx_dtype(tensor) is not None

    @classmethod
    def payload_like(cls, x):
        """An uninitialised payload buffer for x, of x's kind and device."""
        from .mx import payload_bytes
        size = payload_bytes(int(x.numel()) if _is_torch(x) else int(x.size), cls.FMT)
        if _is_torch(x):
            import torch
            return torch.empty(size, dtype=torch.uint8, device=x.device)
        return np.empty(size, dtype=np.uint8)

    @classmethod
    def payload_nbytes(cls, n: int) -> int:
        """The bytes of the payload of ``n`` elements."""
        from .mx import payload_bytes
        return payload_bytes(n, cls.FMT)

    @classmethod
    def init_payload(cls, n: int):
        """The payload of ``n`` zeros, a new uint8 array: the header ``{bits,
        n}`` and zeros — what a key's init push carries."""
        from .mx import bits_of
        zero = np.zeros(cls.payload_nbytes(n), dtype=np.uint8)
        zero[0:4] = np.array([bits_of(cls.FMT)], dtype="<u4").view(np.uint8)
        zero[4:12] = np.array([int(n)], dtype="<u8").view(np.uint8)
        return zero

    residual_like = classmethod(_ErrorFeedback.residual_like.__func__)

    @classmethod
    def compress(cls, tensor):
        """The stateless form: one step from a zero residual, which is
        dropped.  ``ctx`` is ``(dtype, shape)``."""
        ctx = (tensor.dtype, tuple(tensor.shape))
        if not cls.compresses(tensor):
            return tensor, ctx
        flat = tensor.contiguous() if _is_torch(tensor) else np.ascontiguousarray(tensor)
        return cls.compress_ef_into(cls.payload_like(flat), cls.residual_like(flat), flat), ctx

    decompress = classmethod(OneBitEFCompressor.decompress.__func__)

    @classmethod
    def compress_ef_into(cls, payload, residual, tensor, plans: CastPlanCache | None = None):
        """``payload, residual = mx.compress(tensor, residual, FMT)``, the
        residual in place; returns ``payload``."""
        cls.compress_many_ef_into([payload], [residual], [tensor], plans)
        return payload

    @classmethod
    def compress_many_ef_into(cls, payloads, residuals, tensors,
                              plans: CastPlanCache | None = None):
        """``compress_ef_into`` for every i, the device tensors as one
        block-scaled plan per device (ONE launch); returns ``payloads``."""
        from . import mx
        if len(payloads) != len(tensors) or len(residuals) != len(tensors):
            raise ValueError("compress_many_ef_into: as many payloads and residuals as tensors")
        name, groups = f"mx{cls.FMT}_ef", {}
        for i, (p, r, t) in enumerate(zip(payloads, residuals, tensors)):
            if not cls.compresses(t) or not _is_f32(r):
                raise ValueError(f"{name} needs float32, float16 or bfloat16 tensors and "
                                 f"float32 residuals")
            dev = [_on_device(x) for x in (p, r, t)]
            if any(dev) != all(dev):
                raise ValueError(f"{name}: tensor {i}'s operands live in one place, a device "
                                 f"or the host")
            if dev[0]:
                cls._check_device_segment(i, t, r, payload=p)
                groups.setdefault((t.device, _mx_dtype(t)), []).append(
                    (t.reshape(-1), r.reshape(-1), p))
                continue
            ra, ga, pa = _mx_host(r), _mx_host(t), _payload_array(p)
            if ra.size != ga.size or pa.size != mx.payload_bytes(ga.size, cls.FMT):
                raise ValueError(f"{name}: tensor {i}'s operands differ in size")
            pa[:], ra[:] = mx.compress(ga, ra, cls.FMT, _is_bf16(t))
        _run_by_dtype(groups, plans, lambda cache, segs, dt: cache.get_mx(segs, cls.FMT, dt),
                      lambda plan, stream: plan.compress(stream=stream))
        return payloads

    @classmethod
    def decompress_into(cls, out, payload, divisor: int = 1, plans: CastPlanCache | None = None):
        """``out = mx.decode(payload)`` (divided by ``divisor`` above 1): the
        one-source fold; returns ``out``."""
        cls.fold_many_into([out], [[payload]], divisor, plans)
        return out

    @classmethod
    def fold_many_into(cls, outs, payload_lists, divisor: int = 1,
                       plans: CastPlanCache | None = None):
        """``outs[i] = mx.fold(payload_lists[i], outs[i].size, FMT, divisor)``
        for every i — every list of the same length N, 1..16 — the device
        tensors as one block-scaled fold plan per device (ONE launch); returns
        ``outs``."""
        from . import mx
        if len(outs) != len(payload_lists):
            raise ValueError("fold_many_into: as many payload lists as outputs")
        if int(divisor) < 1:
            raise ValueError(f"divisor {divisor} < 1")
        nsrc = len(payload_lists[0]) if payload_lists else 1
        if not 1 <= nsrc <= mx.MAX_SRCS or any(len(ps) != nsrc for ps in payload_lists):
            raise ValueError(f"fold_many_into: every output takes the same 1..{mx.MAX_SRCS} "
                             f"payloads")
        name, groups = f"mx{cls.FMT}_ef", {}
        for i, (o, ps) in enumerate(zip(outs, payload_lists)):
            if _mx_dtype(o) is None:
                raise ValueError(f"{name}: output {i} must be float32, float16 or bfloat16, "
                                 f"got {o.dtype}")
            dev = [_on_device(x) for x in [o] + list(ps)]
            if any(dev) != all(dev):
                raise ValueError(f"{name}: output {i} and its payloads live in one place, a "
                                 f"device or the host")
            if dev[0]:
                for p in ps:
                    cls._check_device_segment(i, o, payload=p)
                groups.setdefault((o.device, _mx_dtype(o)), []).append((o.reshape(-1), list(ps)))
                continue
            oa = _mx_host(o)
            oa[:] = mx.fold([_payload_array(p) for p in ps], oa.size, cls.FMT, divisor,
                            _MX_OUT[_mx_dtype(o)])
        _run_by_dtype(groups, plans,
                      lambda cache, segs, dt: cache.get_mx_fold(segs, nsrc, cls.FMT, dt),
                      lambda plan, stream: plan.launch(int(divisor), stream=stream))
        return outs

    @classmethod
    def refold_many_into(cls, out_payloads, residuals, payload_lists,
                         plans: CastPlanCache | None = None):
        """The server round: ``out_payloads[i], residuals[i] =
        mx.refold(payload_lists[i], residuals[i].size, residuals[i], FMT)`` for
        every i — every list of the same length N, 1..16, the float32 residual
        in place — the device tensors as one block-scaled refold plan per
        device (ONE launch, the folded sum never written); returns
        ``out_payloads``."""
        from . import mx
        if len(out_payloads) != len(payload_lists) or len(residuals) != len(payload_lists):
            raise ValueError("refold_many_into: as many output payloads and residuals as "
                             "payload lists")
        nsrc = len(payload_lists[0]) if payload_lists else 1
        if not 1 <= nsrc <= mx.MAX_SRCS or any(len(ps) != nsrc for ps in payload_lists):
            raise ValueError(f"refold_many_into: every segment takes the same "
                             f"1..{mx.MAX_SRCS} payloads")
        name, groups = f"mx{cls.FMT}_ef", {}
        for i, (o, r, ps) in enumerate(zip(out_payloads, residuals, payload_lists)):
            if not _is_f32(r):
                raise ValueError(f"{name}: residual {i} must be float32, got {r.dtype}")
            dev = [_on_device(x) for x in [o, r] + list(ps)]
            if any(dev) != all(dev):
                raise ValueError(f"{name}: segment {i}'s operands live in one place, a device "
                                 f"or the host")
            if dev[0]:
                for p in [o] + list(ps):
                    cls._check_device_segment(i, r, payload=p)
                groups.setdefault(r.device, []).append((list(ps), r.reshape(-1), o))
                continue
            ra, oa = _mx_host(r), _payload_array(o)
            if oa.size != mx.payload_bytes(ra.size, cls.FMT):
                raise ValueError(f"{name}: segment {i}'s operands differ in size")
            oa[:], ra[:] = mx.refold([_payload_array(p) for p in ps], ra.size, ra, cls.FMT)
        OneBitEFCompressor._run(groups, plans,
                                lambda cache, segs: cache.get_mx_refold(segs, nsrc, cls.FMT),
                                lambda plan, stream: plan.launch(stream=stream))
        return out_payloads

    @classmethod
    def _check_device_segment(cls, i: int, tensor, resid=None, payload=None) -> None:
        """One device segment: contiguous operands of one size and a flat
        uint8 payload of the payload's size, all on one device."""
        import torch
        from .mx import payload_bytes
        for x in (tensor, resid):
            if x is not None and (not x.is_contiguous() or x.device != tensor.device
                                  or x.numel() != tensor.numel()):
                raise ValueError(f"mx{cls.FMT}_ef: tensor {i} needs contiguous operands of one "
                                 f"size on one device")
        size = payload_bytes(tensor.numel(), cls.FMT)
        if payload.dtype != torch.uint8 or not payload.is_contiguous() or payload.dim() != 1 \
                or payload.device != tensor.device or payload.numel() != size:
            raise ValueError(f"mx{cls.FMT}_ef: tensor {i}'s payload must be a flat uint8 tensor "
                             f"of {size} bytes on {tensor.device}")


class MXFP4EFCompressor(MXFP8EFCompressor):
    """``MXFP8EFCompressor`` over OCP e2m1 codes: 4.25 bits an element."""

    FMT = "fp4"


class MXFP8SRCompressor(Compressor):
    """float32, float16 and bfloat16 tensors travel in ``mxfp8_ef``'s blocks with no residual: a code
    is rounded up with a probability equal to the dropped fraction, under bits
    that are a pure function of ``(key, step, element index)``
    (``prophet_amd/mx_sr.py`` is the definition).  The
    ``ROTATE`` variants (``mxfp8_rht_sr``, ``mxfp4_rht_sr``) put every whole
    block through a random-sign Hadamard rotation first, under a ``rot_key``
    all workers of a tensor share (``mx_sr.rotation_key``), and undo it once in
    the fold, which then takes the compress's ``rot_keys`` and ``step``.
    Device tensors go through plans (``byteps_reduce_mx_sr_*``,
    ``byteps_reduce_mx_rht_fold_*``, ``prophet_amd/csrc/bpsr_k_mx_sr.hip``; the
    unrotated fold is ``mxfp8_ef``'s): ONE launch per device either way; CPU
    tensors and numpy arrays go through ``mx_sr.py``, byte for byte the same.
    A float16 or bfloat16 tensor gives the payload of its exact float32 upcast
    and a fold converts its float32 result once to the output's type
    (``prophet_amd/csrc/bpsr_k_mx_half.hip``).  Everything
    else passes through.

    There is no server round for these wires: ``Worker.init_tensor`` refuses
    them over every front end."""

    STOCHASTIC = True
    PACKED = True
    FMT = "fp8"
    ROTATE = False

    compresses = classmethod(MXFP8EFCompressor.compresses.__func__)
    payload_like = classmethod(MXFP8EFCompressor.payload_like.__func__)

    @classmethod
    def _name(cls) -> str:
        return f"mx{cls.FMT}{'_rht' if cls.ROTATE else ''}_sr"

    @classmethod
    def compress(cls, tensor, key: int = 0, step: int = 0, rot_key: int = 0):
        """One payload under ``(key, step, rot_key)``; ``ctx`` is ``(dtype,
        shape, rot_key, step)``."""
        ctx = (tensor.dtype, tuple(tensor.shape), rot_key, step)
        if not cls.compresses(tensor):
            return tensor, ctx
        flat = tensor.contiguous() if _is_torch(tensor) else np.ascontiguousarray(tensor)
        return cls.compress_sr_into(cls.payload_like(flat), flat, key, step, rot_key), ctx

    @classmethod
    def decompress(cls, payload, ctx):
        dtype, shape, rot_key, step = ctx
        if payload.dtype == dtype:
            return payload
        if _is_torch(payload):
            import torch
            out = torch.empty(shape, dtype=dtype, device=payload.device)
        else:
            out = np.empty(shape, dtype=dtype)
        return cls.decompress_into(out, payload, 1, rot_key, step)

    @classmethod
    def compress_sr_into(cls, payload, tensor, key: int, step: int, rot_key: int = 0,
                         plans: CastPlanCache | None = None):
        """``payload = mx_sr.compress(tensor, FMT, key, step, ROTATE,
        rot_key)``; returns ``payload``."""
        cls.compress_many_sr_into([payload], [tensor], [key], step, [rot_key], plans)
        return payload

    @classmethod
    def compress_many_sr_into(cls, payloads, tensors, keys, step: int, rot_keys=None,
                              plans: CastPlanCache | None = None):
        """``compress_sr_into`` for every i, the device tensors as one plan per
        device (ONE launch); returns ``payloads``."""
        from . import mx, mx_sr
        rot_keys = [0] * len(tensors) if rot_keys is None else list(rot_keys)
        if not len(payloads) == len(keys) == len(rot_keys) == len(tensors):
            raise ValueError("compress_many_sr_into: as many payloads and keys as tensors")
        name, groups = cls._name(), {}
        for i, (p, t, k, rk) in enumerate(zip(payloads, tensors, keys, rot_keys)):
            if not cls.compresses(t):
                raise ValueError(f"{name} needs float32, float16 or bfloat16 tensors")
            k, rk = int(k) & 0xffffffff, int(rk) & 0xffffffff
            if _on_device(p) != _on_device(t):
                raise ValueError(f"{name}: tensor {i}'s operands live in one place, a device "
                                 f"or the host")
            if _on_device(t):
                cls._check_device_segment(i, t, p)
                groups.setdefault((t.device, _mx_dtype(t)), []).append((t.reshape(-1), p, k, rk))
                continue
            ga, pa = _mx_host(t), _payload_array(p)
            if pa.size != mx.payload_bytes(ga.size, cls.FMT):
                raise ValueError(f"{name}: tensor {i}'s operands differ in size")
            pa[:] = mx_sr.compress(ga, cls.FMT, k, step, cls.ROTATE, rk, _is_bf16(t))
        _run_by_dtype(
            groups, plans,
            lambda cache, segs, dt: cache.get_mx_sr(segs, cls.FMT, cls.ROTATE, dt),
            lambda plan, stream: plan.compress(step, stream=stream))
        return payloads

    @classmethod
    def decompress_into(cls, out, payload, divisor: int = 1, rot_key: int = 0, step=None,
                        plans: CastPlanCache | None = None):
        """The one-source fold; returns ``out``."""
        cls.fold_many_into([out], [[payload]], divisor, [rot_key], step, plans)
        return out

    @classmethod
    def fold_many_into(cls, outs, payload_lists, divisor: int = 1, rot_keys=None, step=None,
                       plans: CastPlanCache | None = None):
        """``outs[i] = mx_sr.fold(payload_lists[i], outs[i].size, FMT, divisor,
        ROTATE, rot_keys[i], step)`` for every i — every list of the same
        length N, 1..16 — the device tensors as one fold plan per device (ONE
        launch); returns ``outs``.  The unrotated compressors take
        ``mxfp8_ef``'s fold plan and read neither ``rot_keys`` nor ``step``."""
        from . import mx, mx_sr
        if not cls.ROTATE:
            return MXFP8EFCompressor.fold_many_into.__func__(cls, outs, payload_lists, divisor,
                                                             plans)
        if step is None:
            raise ValueError(f"{cls._name()}: a rotated fold takes the compress's step")
        rot_keys = [0] * len(outs) if rot_keys is None else list(rot_keys)
        if len(outs) != len(payload_lists) or len(rot_keys) != len(outs):
            raise ValueError("fold_many_into: as many payload lists and rotation keys as outputs")
        if int(divisor) < 1:
            raise ValueError(f"divisor {divisor} < 1")
        nsrc = len(payload_lists[0]) if payload_lists else 1
        if not 1 <= nsrc <= mx.MAX_SRCS or any(len(ps) != nsrc for ps in payload_lists):
            raise ValueError(f"fold_many_into: every output takes the same 1..{mx.MAX_SRCS} "
                             f"payloads")
        name, groups = cls._name(), {}
        for i, (o, ps, rk) in enumerate(zip(outs, payload_lists, rot_keys)):
            if _mx_dtype(o) is None:
                raise ValueError(f"{name}: output {i} must be float32, float16 or bfloat16, "
                                 f"got {o.dtype}")
            dev = [_on_device(x) for x in [o] + list(ps)]
            if any(dev) != all(dev):
                raise ValueError(f"{name}: output {i} and its payloads live in one place, a "
                                 f"device or the host")
            rk = int(rk) & 0xffffffff
            if dev[0]:
                for p in ps:
                    cls._check_device_segment(i, o, p)
                groups.setdefault((o.device, _mx_dtype(o)), []).append(
                    (o.reshape(-1), list(ps), rk))
                continue
            oa = _mx_host(o)
            oa[:] = mx_sr.fold([_payload_array(p) for p in ps], oa.size, cls.FMT, divisor, True,
                               rk, step, _MX_OUT[_mx_dtype(o)])
        _run_by_dtype(
            groups, plans,
            lambda cache, segs, dt: cache.get_mx_rht_fold(segs, nsrc, cls.FMT, dt),
            lambda plan, stream: plan.launch(int(divisor), step, stream=stream))
        return outs

    @classmethod
    def _check_device_segment(cls, i: int, tensor, payload=None, **_) -> None:
        """One device segment: a contiguous tensor and a flat uint8 payload of
        the payload's size on its device."""
        import torch
        from .mx import payload_bytes
        size = payload_bytes(tensor.numel(), cls.FMT)
        if not tensor.is_contiguous() or payload.dtype != torch.uint8 \
                or not payload.is_contiguous() or payload.dim() != 1 \
                or payload.device != tensor.device or payload.numel() != size:
            raise ValueError(f"{cls._name()}: tensor {i} must be contiguous and its payload a "
                             f"flat uint8 tensor of {size} bytes on {tensor.device}")


class MXFP4SRCompressor(MXFP8SRCompressor):
    """``MXFP8SRCompressor`` over OCP e2m1 codes."""

    FMT = "fp4"


class MXFP8RHTSRCompressor(MXFP8SRCompressor):
    """``MXFP8SRCompressor`` with every whole block rotated."""

    ROTATE = True


class MXFP4RHTSRCompressor(MXFP8SRCompressor):
    """``MXFP4SRCompressor`` with every whole block rotated."""

    FMT = "fp4"
    ROTATE = True


class PowerSGDEFCompressor(Compressor):
    """float32 tensors of two or more dimensions travel as the two factors of
    a rank-r approximation, with error feedback (``prophet_amd/powersgd.py`` is
    the definition).  Device tensors go through PowerSGD plans
    (``byteps_reduce_powersgd_*``, ``prophet_amd/csrc/bpsr_k_powersgd.hip``):
    each of the four phases is one fixed sequence of launches per device over
    every tensor; CPU tensors and numpy arrays go through ``powersgd.py``.  The
    two projections are held to a dot product's error bound, not to the host's
    bytes; the residual's ``g + R``, ``finish`` and determinism are pinned.

    The wire is ``P`` and ``Q`` themselves, plain float32:
    ``powersgd.push_pull_many`` is the round, and ``Worker.init_tensor`` refuses
    this compressor.  The four ``*_many`` take the same ``tensors`` and
    ``states`` (and ``outs``, the tensors themselves unless given), which is how
    a cached plan is found again."""

    ERROR_FEEDBACK = True
    PACKED = True                         # no element-wise wire dtype: init_tensor refuses it

    @staticmethod
    def compresses(tensor, rank: int = 4) -> bool:
        from .powersgd import compresses
        return compresses(tensor, rank)

    @classmethod
    def state_like(cls, tensor, rank: int, seed: int):
        """A ``powersgd.State`` of the tensor's kind and device — a zero
        residual, the warm start ``init_q(m, rank, seed)``, zeroed ``P`` and
        ``Qn`` — or None for a tensor that does not compress."""
        from . import powersgd
        if not cls.compresses(tensor, rank):
            return None
        n, m = powersgd.shape_of(tensor)
        q = powersgd.init_q(m, rank, seed)
        if _is_torch(tensor):
            import torch
            z = lambda *shape: torch.zeros(*shape, dtype=torch.float32,      # noqa: E731
                                           device=tensor.device)
            return powersgd.State(rank, n, m, z(n, m), torch.from_numpy(q).to(tensor.device),
                                  z(n, rank), z(m, rank))
        z = lambda *shape: np.zeros(shape, np.float32)                       # noqa: E731
        return powersgd.State(rank, n, m, z(n, m), q, z(n, rank), z(m, rank))

    @classmethod
    def compress(cls, tensor):
        raise ValueError("powersgd_ef has no stateless form: use powersgd.push_pull_many")

    decompress = compress

    @classmethod
    def _phase(cls, name, tensors, states, plans, outs, host) -> None:
        """Phase ``name`` of every (tensor, state): the device ones as one plan
        per device and rank, the host ones through ``host(g, out, state)``."""
        outs = tensors if outs is None else outs
        if len(states) != len(tensors) or len(outs) != len(tensors):
            raise ValueError(f"{name}_many: as many states and outputs as tensors")
        groups = {}
        for i, (t, o, st) in enumerate(zip(tensors, outs, states)):
            ops = (t, o, st.R, st.Q, st.P, st.Qn)
            if not cls.compresses(t, st.rank) or not all(_is_f32(x) for x in ops):
                raise ValueError(f"powersgd_ef: tensor {i} does not compress at rank {st.rank}")
            dev = [_on_device(x) for x in ops]
            if any(dev) != all(dev):
                raise ValueError(f"powersgd_ef: tensor {i}'s operands live in one place, a "
                                 f"device or the host")
            n, m = st.n, st.m
            want = ((n * m, (t, o, st.R)), (n * st.rank, (st.P,)), (m * st.rank, (st.Q, st.Qn)))
            if dev[0]:
                for size, xs in want:
                    if any(x.numel() != size or not x.is_contiguous() or x.device != t.device
                           for x in xs):
                        raise ValueError(f"powersgd_ef: tensor {i} needs contiguous operands of "
                                         f"a {n} x {m} matrix at rank {st.rank} on {t.device}")
                groups.setdefault((t.device, st.rank), []).append(
                    (t, st.R, st.P, st.Q, st.Qn, o, n, m))
                continue
            if any(int(np.asarray(x).size) != size for size, xs in want for x in xs):
                raise ValueError(f"powersgd_ef: tensor {i}'s operands differ in size")
            # the phases write through reshaped views: a copy would lose the result
            if not all(x.is_contiguous() if _is_torch(x) else x.flags["C_CONTIGUOUS"]
                       for x in ops):
                raise ValueError(f"powersgd_ef: tensor {i} needs contiguous operands")
            view = lambda x, rows: (x.detach().numpy() if _is_torch(x) else x).reshape(rows, -1)  # noqa: E731
            host(view(t, n), view(o, n), st, view)
        for (device, rank), segs in groups.items():
            OneBitEFCompressor._run({device: segs}, plans,
                                    lambda cache, sg: cache.get_powersgd(sg, rank),
                                    lambda plan, stream: getattr(plan, name)(stream=stream))

    @classmethod
    def project_p_many(cls, tensors, states, plans: CastPlanCache | None = None, outs=None):
        """``state.P = powersgd.project_p(tensor, state.R, state.Q)`` for every i."""
        from . import powersgd

        def host(g, o, st, view):
            view(st.P, st.n)[:] = powersgd.project_p(g, view(st.R, st.n), view(st.Q, st.m))
        cls._phase("project_p", tensors, states, plans, outs, host)

    @classmethod
    def orthogonalize_many(cls, tensors, states, plans: CastPlanCache | None = None, outs=None):
        """``powersgd.orthogonalize(state.P)`` for every i, on the aggregated ``P``."""
        from . import powersgd
        cls._phase("orthogonalize", tensors, states, plans, outs,
                   lambda g, o, st, view: powersgd.orthogonalize(view(st.P, st.n)))

    @classmethod
    def project_q_many(cls, tensors, states, plans: CastPlanCache | None = None, outs=None):
        """``state.Qn = powersgd.project_q(state.R, state.P)`` for every i."""
        from . import powersgd

        def host(g, o, st, view):
            view(st.Qn, st.m)[:] = powersgd.project_q(view(st.R, st.n), view(st.P, st.n))
        cls._phase("project_q", tensors, states, plans, outs, host)

    @classmethod
    def finish_many(cls, tensors, states, plans: CastPlanCache | None = None, outs=None):
        """``powersgd.finish(out, state.R, state.P, state.Qn)`` for every i, on
        the aggregated ``Qn``, which then becomes the warm start: ``state.Q`` and
        ``state.Qn`` change places."""
        from . import powersgd
        cls._phase("finish", tensors, states, plans, outs,
                   lambda g, o, st, view: powersgd.finish(o, view(st.R, st.n), view(st.P, st.n),
                                                          view(st.Qn, st.m)))
        for st in states:
            st.Q, st.Qn = st.Qn, st.Q


class Compression:
    """Optional gradient compression used during push_pull."""

    none = NoneCompressor
    fp16 = FP16Compressor
    bf16 = BF16Compressor
    fp16_ef = FP16EFCompressor
    bf16_ef = BF16EFCompressor
    fp16_sr = FP16SRCompressor
    bf16_sr = BF16SRCompressor
    onebit_ef = OneBitEFCompressor
    topk_ef = TopKEFCompressor
    mxfp8_ef = MXFP8EFCompressor
    mxfp4_ef = MXFP4EFCompressor
    mxfp8_sr = MXFP8SRCompressor
    mxfp4_sr = MXFP4SRCompressor
    mxfp8_rht_sr = MXFP8RHTSRCompressor
    mxfp4_rht_sr = MXFP4RHTSRCompressor
    powersgd_ef = PowerSGDEFCompressor


__all__ = ["Compressor", "NoneCompressor", "FP16Compressor", "BF16Compressor",
           "FP16EFCompressor", "BF16EFCompressor", "FP16SRCompressor", "BF16SRCompressor",
           "OneBitEFCompressor", "TopKEFCompressor", "MXFP8EFCompressor", "MXFP4EFCompressor",
           "MXFP8SRCompressor", "MXFP4SRCompressor", "MXFP8RHTSRCompressor",
           "MXFP4RHTSRCompressor", "PowerSGDEFCompressor", "Compression", "CastPlanCache", "decompress_stats", "clip_record", "ClipValues"]
