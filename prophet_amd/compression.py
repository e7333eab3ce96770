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
        plan = self._plans.get(key)
        if plan is not None:
            self._plans.move_to_end(key)
            return plan
        plan = _new_plan(wide_dtype, pairs, wire_dtype)
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
        plan = self._plans.get(key)
        if plan is not None:
            self._plans.move_to_end(key)
            return plan
        plan = _new_sgd_plan(triples, wire_dtype)
        self.built += 1
        self._plans[key] = plan
        while len(self._plans) > self.capacity:
            _, old = self._plans.popitem(last=False)
            old.close()
        return plan

    def close(self) -> None:
        while self._plans:
            _, plan = self._plans.popitem(last=False)
            plan.close()


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


class Compression:
    """Optional gradient compression used during push_pull."""

    none = NoneCompressor
    fp16 = FP16Compressor
    bf16 = BF16Compressor
    fp16_ef = FP16EFCompressor
    bf16_ef = BF16EFCompressor
    fp16_sr = FP16SRCompressor
    bf16_sr = BF16SRCompressor


__all__ = ["Compressor", "NoneCompressor", "FP16Compressor", "BF16Compressor",
           "FP16EFCompressor", "BF16EFCompressor", "FP16SRCompressor", "BF16SRCompressor",
           "Compression", "CastPlanCache", "decompress_stats", "clip_record", "ClipValues"]
