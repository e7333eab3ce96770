"""torch operator surface of the reduce path (``torch.ops.bpsr.*``).

What byteps/torch would call on device tensors in place of the host
``CpuReducer`` (byteps/common/cpu_reducer.h:49-58), registered with
``torch.library`` so the ops order with the caller's torch work (they run on
the current stream of the tensors' device), show up in profiles under their
own names, and trace through ``torch.compile`` (fake implementations give the
output metadata without touching data):

====================================  ===========================================
op                                    reference / C ABI
====================================  ===========================================
``bpsr::sum_(dst, src)``              ``CpuReducer::sum(dst, src, len, dtype)``,
                                      cpu_reducer.cc:57-83 -> byteps_reduce_sum
``bpsr::sum3_(dst, a, b)``            ``CpuReducer::sum(dst, a, b, len, dtype)``,
                                      cpu_reducer.cc:130-162 -> byteps_reduce_sum3
``bpsr::copy_(dst, src)``             ``CpuReducer::copy``, cpu_reducer.cc:209-220
``bpsr::sum_n(srcs, mode) -> out``    one server round, server.cc:216-273
                                      (left fold in list order) -> byteps_reduce_sum_n
``bpsr::sum_n_out(dst, srcs, mode)``  the same into ``dst`` (``dst`` may be
                                      ``srcs[0]``: the zero-copy accumulator)
``bpsr::compress_fp16(src) -> out``   ``FP16Compressor.compress``,
                                      byteps/torch/compression.py
                                      -> byteps_reduce_compress_to
``bpsr::compress_fp16_out(dst, src)`` the same into a preallocated fp16 ``dst``
``bpsr::decompress_fp16_out(dst,      ``FP16Compressor.decompress`` fused with
src, divisor)``                       average's divide on the fp16 value
                                      -> byteps_reduce_decompress_from
``bpsr::compress_bf16(src) -> out``   ``BF16Compressor.compress`` (build
                                      extension: f32 / f64 / fp16 as bf16)
                                      -> byteps_reduce_compress_to
``bpsr::compress_bf16_out(dst, src)`` the same into a preallocated bf16 ``dst``
``bpsr::decompress_bf16_out(dst,      ``BF16Compressor.decompress`` fused with
src, divisor)``                       average's divide on the bf16 value
                                      -> byteps_reduce_decompress_from
``bpsr::compress_fp16_ef_out(dst,     error-feedback compress (``Compression.
resid, src)``                         fp16_ef``): ``dst = fp16(src + resid)``,
                                      ``resid`` keeps the rounding error;
                                      mutates both -> byteps_reduce_compress_ef
``bpsr::compress_bf16_ef_out(dst,     the same over the bf16 wire
resid, src)``
``bpsr::compress_fp16_sr_out(dst,     stochastic-rounding compress
src, key, step)``                     (``Compression.fp16_sr``): the bytes of
                                      ``prophet_amd.sr.sr_round``; mutates
                                      ``dst`` -> byteps_reduce_compress_sr
``bpsr::compress_bf16_sr_out(dst,     the same over the bf16 wire
src, key, step)``
====================================  ===========================================

Tensors must be contiguous, on one CUDA (HIP) device, of one dtype among the
reference's (+ bf16) and of equal size; ``len`` is the whole tensor.  There is
no CPU kernel: a CPU tensor raises (no silent fallback).
"""
from __future__ import annotations

from typing import List

import torch

from .dtypes import DType, from_torch
from .reducer import MODE_REFERENCE, GpuReducer, ReduceError, EARGS, EDTYPE

_RED = None


def _red() -> GpuReducer:
    global _RED
    if _RED is None:
        _RED = GpuReducer()
    return _RED


def _check_same(dst: torch.Tensor, others) -> int:
    for t in (dst, *others):
        if t.device.type != "cuda":
            raise ReduceError(EARGS, f"bpsr ops need device tensors, got {t.device}")
        if not t.is_contiguous():
            raise ReduceError(EARGS, "bpsr ops need contiguous tensors")
        if t.dtype != dst.dtype or t.numel() != dst.numel() or t.device != dst.device:
            raise ReduceError(EARGS, "bpsr ops need tensors of one dtype, size and device")
    return dst.numel() * dst.element_size()


def _stream(t: torch.Tensor) -> int:
    return int(torch.cuda.current_stream(t.device).cuda_stream)


@torch.library.custom_op("bpsr::sum_", mutates_args=("dst",), device_types="cuda")
def sum_(dst: torch.Tensor, src: torch.Tensor) -> None:
    n = _check_same(dst, [src])
    _red().sum(dst, src, n, from_torch(dst.dtype), stream=_stream(dst))


@torch.library.custom_op("bpsr::sum3_", mutates_args=("dst",), device_types="cuda")
def sum3_(dst: torch.Tensor, a: torch.Tensor, b: torch.Tensor) -> None:
    n = _check_same(dst, [a, b])
    _red().sum3(dst, a, b, n, from_torch(dst.dtype), stream=_stream(dst))


@torch.library.custom_op("bpsr::copy_", mutates_args=("dst",), device_types="cuda")
def copy_(dst: torch.Tensor, src: torch.Tensor) -> None:
    n = _check_same(dst, [src])
    _red().copy(dst, src, n, stream=_stream(dst))


@torch.library.custom_op("bpsr::sum_n_out", mutates_args=("dst",), device_types="cuda")
def sum_n_out(dst: torch.Tensor, srcs: List[torch.Tensor], mode: int = MODE_REFERENCE) -> None:
    if not srcs:
        raise ReduceError(EARGS, "sum_n needs at least one source")
    n = _check_same(dst, srcs)
    _red().sum_n(dst, list(srcs), n, from_torch(dst.dtype), mode, stream=_stream(dst))


@torch.library.custom_op("bpsr::sum_n", mutates_args=(), device_types="cuda")
def sum_n(srcs: List[torch.Tensor], mode: int = MODE_REFERENCE) -> torch.Tensor:
    if not srcs:
        raise ReduceError(EARGS, "sum_n needs at least one source")
    out = torch.empty_like(srcs[0])
    n = _check_same(out, srcs)
    _red().sum_n(out, list(srcs), n, from_torch(out.dtype), mode, stream=_stream(out))
    return out


_WIDE_OF = {torch.float16: (torch.float32, torch.float64, torch.bfloat16),
            torch.bfloat16: (torch.float32, torch.float64, torch.float16)}
_WIRE_NAME = {torch.float16: "fp16", torch.bfloat16: "bf16"}


def _check_on_device(*tensors) -> None:
    for t in tensors:
        if t.device.type != "cuda":
            raise ReduceError(EARGS, f"bpsr ops need device tensors, got {t.device}")
        if not t.is_contiguous():
            raise ReduceError(EARGS, "bpsr ops need contiguous tensors")


def _check_cast(half: torch.Tensor, wide: torch.Tensor, wire=torch.float16) -> int:
    """Operands of a cast: ``half`` of the wire dtype (fp16 unless named),
    ``wide`` f32 / f64 / the other 2-byte float, as many elements, one device,
    contiguous.  Returns the element count."""
    _check_on_device(half, wide)
    if half.dtype != wire:
        raise ReduceError(EDTYPE, f"the compressed tensor must be {str(wire)[len('torch.'):]}, "
                                  f"got {half.dtype}")
    if wide.dtype not in _WIDE_OF[wire]:
        raise ReduceError(EDTYPE, f"{_WIRE_NAME[wire]} compression of {wide.dtype}")
    if half.numel() != wide.numel() or half.device != wide.device:
        raise ReduceError(EARGS, "bpsr ops need tensors of one size and device")
    return wide.numel()


def _check_cast_ef(dst: torch.Tensor, resid: torch.Tensor, src: torch.Tensor, wire) -> int:
    """Operands of an error-feedback compress: ``_check_cast`` with an f32
    ``src`` and an f32 ``resid`` of its size and device."""
    n = _check_cast(dst, src, wire)
    if src.dtype != torch.float32:
        raise ReduceError(EDTYPE, f"error-feedback compression of {src.dtype} (float32 only)")
    _check_on_device(resid)
    if resid.dtype != torch.float32:
        raise ReduceError(EDTYPE, f"the residual must be float32, got {resid.dtype}")
    if resid.numel() != n or resid.device != src.device:
        raise ReduceError(EARGS, "bpsr ops need tensors of one size and device")
    return n


def _check_cast_sr(dst: torch.Tensor, src: torch.Tensor, wire) -> int:
    """Operands of a stochastic-rounding compress: ``_check_cast`` with an
    f32 ``src``."""
    n = _check_cast(dst, src, wire)
    if src.dtype != torch.float32:
        raise ReduceError(EDTYPE, f"stochastic-rounding compression of {src.dtype} (float32 only)")
    return n


def _cast_ops(wire, name: str) -> dict:
    """Registers the cast ops of one wire format, ``bpsr::compress_<name>`` and
    the rest, with their fakes; returns them by op name."""
    wire_id = from_torch(wire)

    def compress_out(dst: torch.Tensor, src: torch.Tensor) -> None:
        n = _check_cast(dst, src, wire)
        _red().compress(dst, src, n, from_torch(src.dtype), wire_id, stream=_stream(dst))

    def compress(src: torch.Tensor) -> torch.Tensor:
        out = torch.empty(src.shape, dtype=wire, device=src.device)
        compress_out(out, src)
        return out

    def decompress_out(dst: torch.Tensor, src: torch.Tensor, divisor: int = 1) -> None:
        n = _check_cast(src, dst, wire)
        if divisor < 1:
            raise ReduceError(EARGS, f"divisor {divisor} < 1")
        _red().decompress(dst, src, n, from_torch(dst.dtype), wire_id, divisor,
                          stream=_stream(dst))

    def compress_ef_out(dst: torch.Tensor, resid: torch.Tensor, src: torch.Tensor) -> None:
        n = _check_cast_ef(dst, resid, src, wire)
        _red().compress_ef(dst, resid, src, n, DType.FLOAT32, wire_id, stream=_stream(dst))

    def compress_sr_out(dst: torch.Tensor, src: torch.Tensor, key: int, step: int) -> None:
        n = _check_cast_sr(dst, src, wire)
        _red().compress_sr(dst, src, n, key, step, wire_id, stream=_stream(dst))

    def no_output(*args, **kwargs):
        return None

    ops = {}
    for op, fn, mutates, fake in (
            (f"compress_{name}_out", compress_out, ("dst",), no_output),
            (f"compress_{name}", compress, (),
             lambda src: torch.empty(src.shape, dtype=wire, device=src.device)),
            (f"decompress_{name}_out", decompress_out, ("dst",), no_output),
            (f"compress_{name}_ef_out", compress_ef_out, ("dst", "resid"), no_output),
            (f"compress_{name}_sr_out", compress_sr_out, ("dst",), no_output)):
        ops[op] = torch.library.custom_op(f"bpsr::{op}", fn, mutates_args=mutates,
                                          device_types="cuda")
        ops[op].register_fake(fake)
    return ops


# compress_fp16, compress_fp16_out, decompress_fp16_out, compress_fp16_ef_out,
# compress_fp16_sr_out and the same five for bf16, as module-level names
for _wire, _name in ((torch.float16, "fp16"), (torch.bfloat16, "bf16")):
    globals().update(_cast_ops(_wire, _name))


@sum_.register_fake
def _(dst, src):
    return None


@sum3_.register_fake
def _(dst, a, b):
    return None


@copy_.register_fake
def _(dst, src):
    return None


@sum_n_out.register_fake
def _(dst, srcs, mode=MODE_REFERENCE):
    return None


@sum_n.register_fake
def _(srcs, mode=MODE_REFERENCE):
    return torch.empty_like(srcs[0])


OPS = ("sum_", "sum3_", "copy_", "sum_n_out", "sum_n",
       "compress_fp16", "compress_fp16_out", "decompress_fp16_out",
       "compress_bf16", "compress_bf16_out", "decompress_bf16_out",
       "compress_fp16_ef_out", "compress_bf16_ef_out",
       "compress_fp16_sr_out", "compress_bf16_sr_out")

__all__ = ["sum_", "sum3_", "copy_", "sum_n_out", "sum_n", "compress_fp16",
           "compress_fp16_out", "decompress_fp16_out", "compress_bf16",
           "compress_bf16_out", "decompress_bf16_out", "compress_fp16_ef_out",
           "compress_bf16_ef_out", "compress_fp16_sr_out", "compress_bf16_sr_out", "OPS"]
