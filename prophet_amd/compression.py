"""Gradient compression for push_pull (the byteps/torch ``Compression`` surface).

``Compression.none`` and ``Compression.fp16`` keep the reference's interface
(byteps/torch/compression.py): ``compress(tensor) -> (compressed, ctx)`` and
``decompress(tensor, ctx)``, with ``ctx`` the original dtype.  The fp16
compressor casts floating tensors to fp16 before the push and back after the
pull; everything else (integers, tensors that are fp16 already) passes
through as the same object.

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
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np


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


def _on_device(x) -> bool:
    return _is_torch(x) and x.device.type == "cuda"


def _as_host_tensor(x):
    """A CPU torch view of a CPU tensor or numpy array (no copy)."""
    import torch
    return x if _is_torch(x) else torch.from_numpy(x)


class CastPlanCache:
    """The cast plans of the last few iterations, least recently used out
    first.  A plan is found again by its wide dtype and the (wide address,
    fp16 address, element count) of every segment, so a tensor that moved
    misses and gets a new plan.  A cached plan holds its tensors: their
    memory cannot be freed, so no other tensor can appear at a cached
    address while the plan that names it is alive."""

    def __init__(self, capacity: int = 4):
        self.capacity = int(capacity)
        self.built = 0                    # plans created so far
        self._plans: OrderedDict = OrderedDict()

    def __len__(self) -> int:
        return len(self._plans)

    def get(self, wide_dtype: int, pairs):
        """The plan over ``pairs`` of flat ``(wide, half)`` device tensors on
        the current device, built on a miss."""
        key = (int(wide_dtype),) + tuple(
            (int(w.data_ptr()), int(h.data_ptr()), int(w.numel())) for w, h in pairs)
        plan = self._plans.get(key)
        if plan is not None:
            self._plans.move_to_end(key)
            return plan
        plan = _new_plan(wide_dtype, pairs)
        self.built += 1
        self._plans[key] = plan
        while len(self._plans) > self.capacity:
            _, old = self._plans.popitem(last=False)
            old.close()                   # waits for its launches in flight
        return plan

    def close(self) -> None:
        while self._plans:
            _, plan = self._plans.popitem(last=False)
            plan.close()


def _new_plan(wide_dtype: int, pairs):
    from .torch_ops import _red
    return _red().cast_plan([(w, h, int(w.numel())) for w, h in pairs], wide_dtype)


def _cast_many(pairs, compress: bool, divisor: int, plans) -> None:
    """``pairs`` of ``(wide, half)`` tensors or arrays: the device ones as one
    plan launch per (device, wide dtype), the host ones one by one."""
    if int(divisor) < 1:
        raise ValueError(f"divisor {divisor} < 1")
    groups: dict = {}
    for wide, half in pairs:
        if not _on_device(wide) and not _on_device(half):
            if compress:
                FP16Compressor.compress_into(half, wide)
            else:
                FP16Compressor.decompress_into(wide, half, divisor)
            continue
        from .torch_ops import _check_cast
        _check_cast(half, wide)
        groups.setdefault((wide.device, wide.dtype), []).append(
            (wide.reshape(-1), half.reshape(-1)))
    if not groups:
        return
    import torch
    from .dtypes import from_torch
    for (device, dtype), segs in groups.items():
        with torch.cuda.device(device):
            plan = plans.get(from_torch(dtype), segs) if plans is not None \
                else _new_plan(from_torch(dtype), segs)
            stream = torch.cuda.current_stream(device)
            try:
                if compress:
                    plan.compress(stream=stream)
                else:
                    plan.decompress(int(divisor), stream=stream)
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


class FP16Compressor(Compressor):
    """Floating tensors travel as fp16."""

    @staticmethod
    def compresses(tensor) -> bool:
        return _is_floating(tensor) and not _is_half(tensor)

    @staticmethod
    def compress(tensor):
        ctx = tensor.dtype
        if not FP16Compressor.compresses(tensor):
            return tensor, ctx
        import torch
        if _on_device(tensor):
            from . import torch_ops  # noqa: F401  (registers torch.ops.bpsr.*)
            with torch.cuda.device(tensor.device):
                return torch.ops.bpsr.compress_fp16(tensor.contiguous()), ctx
        if _is_torch(tensor):
            return tensor.to(torch.float16), ctx
        return torch.from_numpy(np.ascontiguousarray(tensor)).to(torch.float16).numpy(), ctx

    @staticmethod
    def compress_into(out, tensor):
        """``compress`` into a preallocated fp16 buffer of the same kind and
        element count (push_pull's staging buffer); returns ``out``."""
        import torch
        if _on_device(tensor):
            from . import torch_ops  # noqa: F401
            with torch.cuda.device(tensor.device):
                torch.ops.bpsr.compress_fp16_out(out.reshape(-1), tensor.reshape(-1))
            return out
        _as_host_tensor(out).reshape(-1).copy_(_as_host_tensor(tensor).reshape(-1))
        return out

    @staticmethod
    def decompress(tensor, ctx):
        if ctx is None or tensor.dtype == ctx:
            return tensor
        if _is_torch(tensor):
            if not ctx.is_floating_point:
                return tensor
            import torch
            out = torch.empty(tensor.shape, dtype=ctx, device=tensor.device)
            return FP16Compressor.decompress_into(out, tensor.contiguous())
        if not np.issubdtype(ctx, np.floating):
            return tensor
        out = np.empty(tensor.shape, dtype=ctx)
        return FP16Compressor.decompress_into(out, np.ascontiguousarray(tensor))

    @staticmethod
    def decompress_into(out, compressed, divisor: int = 1):
        """``out[i] = T(compressed[i])``, or ``T(fp16(compressed[i] / divisor))``
        for a divisor above 1 (divide on the fp16 value, then widen), in one
        pass; returns ``out``."""
        if int(divisor) < 1:
            raise ValueError(f"divisor {divisor} < 1")
        import torch
        if _on_device(out):
            from . import torch_ops  # noqa: F401
            with torch.cuda.device(out.device):
                torch.ops.bpsr.decompress_fp16_out(out.reshape(-1), compressed.reshape(-1),
                                                   int(divisor))
            return out
        q = _as_host_tensor(compressed).reshape(-1)
        if int(divisor) > 1:
            q = q.clone().div_(int(divisor))
        _as_host_tensor(out).reshape(-1).copy_(q)
        return out


    @staticmethod
    def compress_many_into(outs, tensors, plans: CastPlanCache | None = None):
        """``compress_into(outs[i], tensors[i])`` for every i, the device
        tensors as one cast-plan launch per (device, dtype); returns ``outs``.
        ``plans`` keeps the plans for the next call over the same tensors;
        without it a plan is built and destroyed here."""
        if len(outs) != len(tensors):
            raise ValueError("compress_many_into: as many outputs as tensors")
        _cast_many(list(zip(tensors, outs)), True, 1, plans)
        return outs

    @staticmethod
    def decompress_many_into(outs, compressed, divisor: int = 1,
                             plans: CastPlanCache | None = None):
        """``decompress_into(outs[i], compressed[i], divisor)`` for every i,
        the device tensors as one cast-plan launch per (device, dtype);
        returns ``outs``."""
        if len(outs) != len(compressed):
            raise ValueError("decompress_many_into: as many outputs as compressed tensors")
        _cast_many(list(zip(outs, compressed)), False, divisor, plans)
        return outs


class Compression:
    """Optional gradient compression used during push_pull."""

    none = NoneCompressor
    fp16 = FP16Compressor


__all__ = ["Compressor", "NoneCompressor", "FP16Compressor", "Compression", "CastPlanCache"]
