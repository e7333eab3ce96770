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
"""
from __future__ import annotations

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


class Compression:
    """Optional gradient compression used during push_pull."""

    none = NoneCompressor
    fp16 = FP16Compressor


__all__ = ["Compressor", "NoneCompressor", "FP16Compressor", "Compression"]
