"""Host-side mirror of the reference reducer surface, over the C ABI.

:class:`GpuReducer` keeps ``CpuReducer``'s method names and argument meaning
(byteps/common/cpu_reducer.h:41-58):

=====================================  =========================================
reference                              here
=====================================  =========================================
``sum(dst, src, len, dtype)``          ``GpuReducer.sum`` -> ``byteps_reduce_sum``
``sum(dst, src1, src2, len, dtype)``   ``GpuReducer.sum3`` -> ``byteps_reduce_sum3``
``copy(dst, src, len)``                ``GpuReducer.copy`` -> ``byteps_reduce_copy``
``FP16Compressor`` (torch front end)   ``GpuReducer.compress_fp16`` / ``decompress_fp16``
``BF16Compressor`` (build extension)   ``GpuReducer.compress`` / ``decompress`` with a wire dtype
``GetDataType(int)``                   ``GpuReducer.GetDataType``
server fold, server.cc:216-273         ``GpuReducer.sum_n`` -> ``byteps_reduce_sum_n``
one Prophet block                      ``GpuReducer.sum_batched``
=====================================  =========================================

``len`` is in BYTES as in the reference.  Operands are device pointers (ints)
or torch CUDA tensors (their ``data_ptr()``); ``stream`` defaults to torch's
current stream on the operand's device so the calls order with the caller's
torch work.  Errors raise :class:`ReduceError` carrying the negative status
(the reference aborts via BPS_CHECK instead, cpu_reducer.cc:79-80).

There is no fallback: if ``libbpsr.so`` is missing the import fails loudly.
"""
from __future__ import annotations

import ctypes
import os
from typing import Sequence

from .dtypes import DType, elem_size

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libbpsr.so")
MAX_SRCS = 32

MODE_REFERENCE = 0
MODE_ACCUM_F32 = 1

OK, EDTYPE, EARGS, EHIP, ERCCL, ETIMEOUT, ECANCELED = 0, -1, -2, -3, -4, -5, -6

_vp, _sz, _int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int

# Every symbol include/bpsr/reduce.h declares (checked by tests/test_abi.py).
EXPORTS = (
    "byteps_reduce_version", "byteps_reduce_init", "byteps_reduce_shutdown",
    "byteps_reduce_sum", "byteps_reduce_sum3", "byteps_reduce_sum_n",
    "byteps_reduce_sum_batched", "byteps_reduce_copy", "byteps_reduce_sync",
    "byteps_reduce_dtype_size", "byteps_reduce_last_error",
    "byteps_reduce_set_tuning", "byteps_reduce_get_tuning",
    "byteps_reduce_plan_create", "byteps_reduce_plan_launch", "byteps_reduce_plan_destroy",
    "byteps_reduce_blockq_create", "byteps_reduce_blockq_config", "byteps_reduce_blockq_launch",
    "byteps_reduce_blockq_release", "byteps_reduce_blockq_status", "byteps_reduce_blockq_destroy",
    "byteps_reduce_blockq_debug", "byteps_reduce_blockq_stream",
    "byteps_reduce_blockq_release_range", "byteps_reduce_blockq_host_releases",
    "byteps_reduce_blockq_release_host", "byteps_reduce_blockq_overlap",
    "byteps_reduce_blockq_join", "byteps_reduce_blockq_release_stream",
    "byteps_reduce_blockq_queue_ids",
    "byteps_reduce_compress_fp16", "byteps_reduce_decompress_fp16",
    "byteps_reduce_cast_plan_create", "byteps_reduce_cast_plan_compress",
    "byteps_reduce_cast_plan_decompress", "byteps_reduce_cast_plan_destroy",
    "byteps_reduce_compress_to", "byteps_reduce_decompress_from",
    "byteps_reduce_cast_plan_create_wire",
    "byteps_reduce_compress_ef", "byteps_reduce_cast_plan_create_ef",
    "byteps_reduce_compress_sr", "byteps_reduce_cast_plan_create_sr",
    "byteps_reduce_cast_plan_compress_sr",
    "byteps_reduce_cast_plan_decompress_stats",
    "byteps_reduce_cast_plan_measure", "byteps_reduce_clip_record",
    "byteps_reduce_cast_plan_decompress_scaled",
    "byteps_reduce_cast_plan_create_sgd", "byteps_reduce_cast_plan_apply_sgd",
)


class BucketDesc(ctypes.Structure):
    """``byteps_bucket_desc`` (include/bpsr/reduce.h)."""
    _fields_ = [("dst", _vp), ("srcs", _vp * MAX_SRCS), ("len", _sz), ("n", _int),
                ("reserved", _int)]


class CastDesc(ctypes.Structure):
    """``byteps_cast_desc`` (include/bpsr/reduce.h)."""
    _fields_ = [("wide", _vp), ("half", _vp), ("nelem", _sz)]


class CastEfDesc(ctypes.Structure):
    """``byteps_cast_ef_desc`` (include/bpsr/reduce.h)."""
    _fields_ = [("wide", _vp), ("half", _vp), ("resid", _vp), ("nelem", _sz)]


class CastSrDesc(ctypes.Structure):
    """``byteps_cast_sr_desc`` (include/bpsr/reduce.h)."""
    _fields_ = [("wide", _vp), ("half", _vp), ("nelem", _sz), ("key", ctypes.c_uint32)]


class CastSgdDesc(ctypes.Structure):
    """``byteps_cast_sgd_desc`` (include/bpsr/reduce.h)."""
    _fields_ = [("param", _vp), ("half", _vp), ("momentum", _vp), ("nelem", _sz)]


class SgdHyper(ctypes.Structure):
    """``byteps_sgd_hyper`` (include/bpsr/reduce.h)."""
    _fields_ = [("lr", ctypes.c_float), ("momentum", ctypes.c_float),
                ("weight_decay", ctypes.c_float), ("nesterov", _int)]


class SrKey(int):
    """A cast-plan segment's stochastic-rounding key: ``(wide, half, nelem,
    SrKey(k))`` asks for an SR plan, where a tensor in that place is an
    error-feedback residual."""


class ReduceError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"byteps_reduce error {code}: {msg}")
        self.code = code


_LIB = None


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    """Load libbpsr.so (once).  Raises if it has not been built."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(path):
        raise ImportError(
            f"{path} not found: build it with `make -C prophet_amd/csrc` "
            "(or __graft_entry__.build()); there is no CPU fallback")
    L = ctypes.CDLL(path)
    L.byteps_reduce_version.restype = _int
    L.byteps_reduce_init.argtypes = [_int]
    L.byteps_reduce_sum.argtypes = [_vp, _vp, _sz, _int, _vp]
    L.byteps_reduce_sum3.argtypes = [_vp, _vp, _vp, _sz, _int, _vp]
    L.byteps_reduce_sum_n.argtypes = [_vp, ctypes.POINTER(_vp), _int, _sz, _int, _int, _vp]
    L.byteps_reduce_sum_batched.argtypes = [ctypes.POINTER(BucketDesc), _int, _int, _int, _vp]
    L.byteps_reduce_copy.argtypes = [_vp, _vp, _sz, _vp]
    L.byteps_reduce_sync.argtypes = [_vp]
    L.byteps_reduce_dtype_size.argtypes = [_int]
    L.byteps_reduce_last_error.restype = ctypes.c_char_p
    L.byteps_reduce_set_tuning.argtypes = [_int, _int, _int, _int]
    L.byteps_reduce_get_tuning.argtypes = [ctypes.POINTER(_int)] * 4
    L.byteps_reduce_plan_create.argtypes = [ctypes.POINTER(BucketDesc), _int, _int, _int,
                                            ctypes.POINTER(_vp)]
    L.byteps_reduce_plan_launch.argtypes = [_vp, _vp]
    L.byteps_reduce_plan_destroy.argtypes = [_vp]
    L.byteps_reduce_blockq_create.argtypes = [ctypes.POINTER(BucketDesc), _int,
                                              ctypes.POINTER(_int), _int, _int, _int,
                                              ctypes.POINTER(_vp)]
    L.byteps_reduce_blockq_config.argtypes = [_vp, _int, ctypes.c_double]
    L.byteps_reduce_blockq_launch.argtypes = [_vp, _vp]
    L.byteps_reduce_blockq_release.argtypes = [_vp, _int, _vp]
    L.byteps_reduce_blockq_release_range.argtypes = [_vp, _int, _int, _vp]
    L.byteps_reduce_blockq_status.argtypes = [_vp, _vp]
    L.byteps_reduce_blockq_host_releases.argtypes = [_vp, _int]
    L.byteps_reduce_blockq_release_host.argtypes = [_vp, _int, _int]
    L.byteps_reduce_blockq_destroy.argtypes = [_vp]
    L.byteps_reduce_blockq_debug.argtypes = [_vp, ctypes.POINTER(ctypes.c_uint32), _int]
    L.byteps_reduce_blockq_stream.argtypes = [_vp, ctypes.POINTER(_vp)]
    L.byteps_reduce_blockq_overlap.argtypes = [_vp, _int]
    L.byteps_reduce_blockq_join.argtypes = [_vp, _vp]
    L.byteps_reduce_blockq_release_stream.argtypes = [_vp, ctypes.POINTER(_vp)]
    L.byteps_reduce_blockq_queue_ids.argtypes = [_vp, ctypes.POINTER(ctypes.c_uint64), _int]
    L.byteps_reduce_compress_fp16.argtypes = [_vp, _vp, _sz, _int, _vp]
    L.byteps_reduce_decompress_fp16.argtypes = [_vp, _vp, _sz, _int, _int, _vp]
    L.byteps_reduce_cast_plan_create.argtypes = [ctypes.POINTER(CastDesc), _int, _int,
                                                 ctypes.POINTER(_vp)]
    L.byteps_reduce_cast_plan_compress.argtypes = [_vp, _vp]
    L.byteps_reduce_cast_plan_decompress.argtypes = [_vp, _int, _vp]
    L.byteps_reduce_cast_plan_destroy.argtypes = [_vp]
    L.byteps_reduce_compress_to.argtypes = [_vp, _vp, _sz, _int, _int, _vp]
    L.byteps_reduce_decompress_from.argtypes = [_vp, _vp, _sz, _int, _int, _int, _vp]
    L.byteps_reduce_cast_plan_create_wire.argtypes = [ctypes.POINTER(CastDesc), _int, _int, _int,
                                                      ctypes.POINTER(_vp)]
    L.byteps_reduce_compress_ef.argtypes = [_vp, _vp, _vp, _sz, _int, _int, _vp]
    L.byteps_reduce_cast_plan_create_ef.argtypes = [ctypes.POINTER(CastEfDesc), _int, _int, _int,
                                                    ctypes.POINTER(_vp)]
    L.byteps_reduce_compress_sr.argtypes = [_vp, _vp, _sz, _int, _int, ctypes.c_uint32,
                                            ctypes.c_uint32, _vp]
    L.byteps_reduce_cast_plan_create_sr.argtypes = [ctypes.POINTER(CastSrDesc), _int, _int, _int,
                                                    ctypes.POINTER(_vp)]
    L.byteps_reduce_cast_plan_compress_sr.argtypes = [_vp, ctypes.c_uint32, _vp]
    L.byteps_reduce_cast_plan_decompress_stats.argtypes = [_vp, _int, _vp, _vp]
    L.byteps_reduce_cast_plan_measure.argtypes = [_vp, _int, _vp, _vp]
    L.byteps_reduce_clip_record.argtypes = [_vp, _int, ctypes.c_double, ctypes.c_double, _vp,
                                            _vp, _vp]
    L.byteps_reduce_cast_plan_decompress_scaled.argtypes = [_vp, _int, _vp, _vp]
    L.byteps_reduce_cast_plan_create_sgd.argtypes = [ctypes.POINTER(CastSgdDesc), _int, _int,
                                                     ctypes.POINTER(_vp)]
    L.byteps_reduce_cast_plan_apply_sgd.argtypes = [_vp, _int, ctypes.POINTER(SgdHyper), _vp,
                                                    _int, _vp]
    _LIB = L
    return L


def _check(rc: int) -> None:
    if rc != OK:
        msg = (_LIB.byteps_reduce_last_error() or b"").decode(errors="replace")
        raise ReduceError(rc, msg)


def _ptr(x) -> int:
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):
        return int(x.data_ptr())
    if x is None:
        return 0
    raise TypeError(f"expected a device pointer or tensor, got {type(x)!r}")


def _fits(length: int, *xs) -> None:
    """Host-side bounds check before a launch: every tensor operand holds at
    least ``length`` bytes (raw pointers carry no size and are the caller's)."""
    for x in xs:
        if hasattr(x, "data_ptr") and hasattr(x, "element_size"):
            have = int(x.numel()) * int(x.element_size())
            if int(length) > have:
                raise ValueError(f"{int(length)}-byte operation on a {have}-byte tensor")


def _fits_cast(nelem: int, half, wide, wide_dtype: int) -> None:
    """``_fits`` for the casts, whose operands differ in element size:
    ``half`` holds ``nelem`` 2-byte values (fp16 or bf16, the wire format),
    ``wide`` as many of ``wide_dtype`` (an unsupported dtype is left to the
    library: EDTYPE)."""
    if int(nelem) < 0:
        raise ValueError(f"negative element count {nelem}")
    _fits(int(nelem) * 2, half)
    if int(wide_dtype) in (DType.FLOAT32, DType.FLOAT64, DType.BFLOAT16, DType.FLOAT16):
        _fits(int(nelem) * elem_size(wide_dtype), wide)


def _stream_of(x, stream):
    if stream is not None:
        return int(getattr(stream, "cuda_stream", stream))
    if hasattr(x, "device") and getattr(x.device, "type", "") == "cuda":
        import torch
        return int(torch.cuda.current_stream(x.device).cuda_stream)
    return 0  # library default: hipStreamPerThread


class GpuReducer:
    """Drop-in for ``byteps::common::CpuReducer`` on device memory."""

    def __init__(self, device: int | None = None):
        self.lib = load_library()
        if device is not None:
            _check(self.lib.byteps_reduce_init(int(device)))

    # cpu_reducer.h:58
    @staticmethod
    def GetDataType(dtype: int) -> DType:
        return DType(dtype)

    def sum(self, dst, src, length: int, dtype: int, stream=None) -> int:
        """In place ``dst += src`` over ``length`` bytes (cpu_reducer.cc:57-83)."""
        _fits(length, dst, src)
        _check(self.lib.byteps_reduce_sum(_ptr(dst), _ptr(src), int(length), int(dtype),
                                          _stream_of(dst, stream)))
        return 0

    def sum3(self, dst, src1, src2, length: int, dtype: int, stream=None) -> int:
        """``dst = src1 + src2`` (cpu_reducer.cc:130-162)."""
        _fits(length, dst, src1, src2)
        _check(self.lib.byteps_reduce_sum3(_ptr(dst), _ptr(src1), _ptr(src2), int(length),
                                           int(dtype), _stream_of(dst, stream)))
        return 0

    def copy(self, dst, src, length: int, stream=None) -> int:
        """``length``-byte device copy (cpu_reducer.cc:209-220)."""
        _fits(length, dst, src)
        _check(self.lib.byteps_reduce_copy(_ptr(dst), _ptr(src), int(length),
                                           _stream_of(dst, stream)))
        return 0

    def compress_fp16(self, dst, src, nelem: int, src_dtype: int, stream=None) -> int:
        """``dst[i] = fp16(src[i])`` for ``nelem`` ELEMENTS of f32, f64 or bf16
        (``compress`` over the FLOAT16 wire; round to nearest even, f64 through
        f32)."""
        return self.compress(dst, src, nelem, src_dtype, DType.FLOAT16, stream)

    def decompress_fp16(self, dst, src, nelem: int, dst_dtype: int, divisor: int = 1,
                        stream=None) -> int:
        """``dst[i] = T(src[i])``, or ``T(fp16(src[i] / divisor))`` for a
        divisor above 1: the average of a compressed push_pull, divided on the
        fp16 value as the reference does (``decompress`` over the FLOAT16
        wire)."""
        return self.decompress(dst, src, nelem, dst_dtype, DType.FLOAT16, divisor, stream)

    def compress(self, dst, src, nelem: int, src_dtype: int, wire_dtype: int,
                 stream=None) -> int:
        """``dst[i] = wire(src[i])`` for ``nelem`` ELEMENTS, the 2-byte wire
        format named (byteps_reduce_compress_to): FLOAT16 takes f32, f64 or
        bf16, BFLOAT16 takes f32, f64 or fp16 (round to nearest even, f64
        through f32, f32 subnormals kept)."""
        _fits_cast(nelem, dst, src, src_dtype)
        _check(self.lib.byteps_reduce_compress_to(_ptr(dst), _ptr(src), int(nelem),
                                                  int(src_dtype), int(wire_dtype),
                                                  _stream_of(dst, stream)))
        return 0

    def decompress(self, dst, src, nelem: int, dst_dtype: int, wire_dtype: int,
                   divisor: int = 1, stream=None) -> int:
        """``dst[i] = T(src[i])``, or ``T(wire(src[i] / divisor))`` for a
        divisor above 1, ``src`` in the named wire format
        (byteps_reduce_decompress_from)."""
        _fits_cast(nelem, src, dst, dst_dtype)
        _check(self.lib.byteps_reduce_decompress_from(_ptr(dst), _ptr(src), int(nelem),
                                                      int(dst_dtype), int(wire_dtype),
                                                      int(divisor), _stream_of(dst, stream)))
        return 0

    def compress_ef(self, dst, resid, src, nelem: int, src_dtype: int, wire_dtype: int,
                    stream=None) -> int:
        """Error-feedback compress (byteps_reduce_compress_ef), one pass over
        ``nelem`` ELEMENTS of FLOAT32: ``c = src + resid``, ``dst = wire(c)``,
        ``resid = c - f32(dst)`` where that is finite and +0.0 elsewhere.
        ``resid`` is f32 and updated in place; any other ``src_dtype`` is
        EDTYPE."""
        _fits_cast(nelem, dst, src, src_dtype)
        _fits(int(nelem) * 4, resid)
        _check(self.lib.byteps_reduce_compress_ef(_ptr(dst), _ptr(resid), _ptr(src), int(nelem),
                                                  int(src_dtype), int(wire_dtype),
                                                  _stream_of(dst, stream)))
        return 0

    def compress_sr(self, dst, src, nelem: int, key: int, step: int, wire_dtype: int,
                    src_dtype: int = DType.FLOAT32, stream=None) -> int:
        """Stochastic-rounding compress (byteps_reduce_compress_sr) of
        ``nelem`` ELEMENTS of FLOAT32: element ``i`` is rounded up with a
        probability equal to the fraction the wire format drops, under 16 bits
        of Philox2x32-10(``i >> 2``, ``step``, ``key``) — the bytes of
        ``prophet_amd.sr.sr_round``.  ``key`` and ``step`` are taken mod 2^32;
        any other ``src_dtype`` is EDTYPE."""
        _fits_cast(nelem, dst, src, src_dtype)
        _check(self.lib.byteps_reduce_compress_sr(_ptr(dst), _ptr(src), int(nelem),
                                                  int(src_dtype), int(wire_dtype),
                                                  int(key) & 0xffffffff, int(step) & 0xffffffff,
                                                  _stream_of(dst, stream)))
        return 0

    def cast_plan(self, segments: Sequence[tuple], wide_dtype: int,
                  wire_dtype: int = DType.FLOAT16) -> "CastPlan":
        """A whole iteration's casts as one launch each way
        (byteps_reduce_cast_plan_*): ``segments`` are ``(wide, half, nelem)``
        triples of tensors or raw pointers, all of ``wide_dtype`` with their
        2-byte sides of ``wire_dtype`` (fp16 unless named).  The plan keeps
        the tensors it was built from alive.

        With ``(wide, half, nelem, resid)`` segments — all of them, FLOAT32
        only — it is an error-feedback plan (byteps_reduce_cast_plan_create_ef):
        ``compress`` adds each f32 residual in and leaves the rounding error
        there, ``decompress`` is the plain one.

        With ``(wide, half, nelem, SrKey(key))`` segments — all of them,
        FLOAT32 only — it is a stochastic-rounding plan
        (byteps_reduce_cast_plan_create_sr): ``compress(step=...)`` writes per
        segment the bytes of ``compress_sr`` under the segment's key,
        ``decompress`` is the plain one."""
        return CastPlan(self.lib, segments, wide_dtype, wire_dtype)

    def sgd_plan(self, segments: Sequence[tuple],
                 wire_dtype: int = DType.FLOAT16) -> "SgdPlan":
        """The SGD step inside the decompress
        (byteps_reduce_cast_plan_create_sgd): ``segments`` are ``(param, half,
        nelem, momentum)`` of tensors or raw pointers — float32 parameters
        and momentum buffers, 2-byte sides of ``wire_dtype``.
        :meth:`SgdPlan.apply` is ONE launch that updates every parameter and
        momentum buffer in place from the wire; no gradient is written."""
        return SgdPlan(self.lib, segments, wire_dtype)

    def clip_record(self, rows, max_norm: float, eps: float = 1e-6, inv_scale=None, out=None,
                    stream=None) -> "ClipRecord":
        """The clip record of statistics rows (byteps_reduce_clip_record; the
        definition: ``compression.clip_record``): ``rows`` is a contiguous
        float64 device tensor of ``[n, 2]`` (or ``2 n``) elements — any
        concatenation of plans' rows — ``inv_scale`` a 1-element float32
        device tensor or None (1).  One small launch on ``stream``; nothing
        synchronises with the host.  Returns a :class:`ClipRecord` (``out``
        if given): 32 bytes on the device with views of its fields.  The
        record holds ``rows`` and ``inv_scale`` until its next use or until
        it is dropped: the launch is asynchronous."""
        import torch
        if not hasattr(rows, "data_ptr") or rows.dtype != torch.float64:
            raise ValueError(f"rows must be a float64 device tensor, got "
                             f"{getattr(rows, 'dtype', type(rows))}")
        if rows.device.type != "cuda" or not rows.is_contiguous() or rows.numel() % 2:
            raise ValueError("rows must be a contiguous device tensor of 2 n elements")
        if inv_scale is not None:
            _check_scalar_f32(inv_scale, "inv_scale", rows.device)
        rec = out if out is not None else ClipRecord(rows.device)
        if not isinstance(rec, ClipRecord):
            raise ValueError(f"out must be a ClipRecord, got {type(out)!r}")
        if rec.tensor.device != rows.device:
            raise ValueError(f"out is on {rec.tensor.device}, rows on {rows.device}")
        rec._keep = (rows, inv_scale)
        _check(self.lib.byteps_reduce_clip_record(
            _ptr(rows), rows.numel() // 2, float(max_norm), float(eps), _ptr(inv_scale),
            _ptr(rec.tensor), _stream_of(rows, stream)))
        return rec

    def sum_n(self, dst, srcs: Sequence, length: int, dtype: int,
              mode: int = MODE_REFERENCE, stream=None) -> int:
        """Left fold ``dst = ((srcs[0] + srcs[1]) + ...)`` in the given order."""
        _fits(length, dst, *srcs)
        arr = (_vp * len(srcs))(*[_ptr(s) for s in srcs])
        _check(self.lib.byteps_reduce_sum_n(_ptr(dst), arr, len(srcs), int(length),
                                            int(dtype), int(mode), _stream_of(dst, stream)))
        return 0

    def sum_batched(self, buckets: Sequence[tuple], dtype: int, mode: int = MODE_REFERENCE,
                    stream=None) -> int:
        """One launch for a block of buckets; each item is ``(dst, srcs, length)``."""
        descs = _descs(buckets)
        first = buckets[0][0] if buckets else None
        _check(self.lib.byteps_reduce_sum_batched(descs, len(buckets), int(dtype), int(mode),
                                                  _stream_of(first, stream)))
        return 0

    def make_plan(self, buckets: Sequence[tuple], dtype: int,
                  mode: int = MODE_REFERENCE) -> "Plan":
        """Upload a block's bucket table once; ``Plan.launch`` is then one
        kernel launch (graph-capturable).  Tensors in ``buckets`` must stay
        alive (and at the same addresses) for the plan's lifetime."""
        return Plan(self.lib, buckets, dtype, mode)

    def make_blockq(self, blocks: Sequence[Sequence[tuple]], dtype: int,
                    mode: int = MODE_REFERENCE) -> "BlockQueue":
        """One iteration's Prophet blocks (in release order; each a list of
        ``(dst, srcs, length)`` buckets) folded by ONE persistent launch per
        iteration that starts each block once it is released
        (``byteps_reduce_blockq_*``)."""
        return BlockQueue(self.lib, blocks, dtype, mode)

    def sync(self, stream=None) -> None:
        _check(self.lib.byteps_reduce_sync(_stream_of(None, stream)))

    def set_tuning(self, vpt: int = 0, nt: int = -1, max_grid: int = 0, occ: int = -1) -> None:
        _check(self.lib.byteps_reduce_set_tuning(vpt, nt, max_grid, occ))

    def get_tuning(self) -> tuple[int, int, int, int]:
        a, b, c, d = _int(), _int(), _int(), _int()
        _check(self.lib.byteps_reduce_get_tuning(ctypes.byref(a), ctypes.byref(b),
                                                 ctypes.byref(c), ctypes.byref(d)))
        return a.value, b.value, c.value, d.value

    @staticmethod
    def dtype_size(dtype: int) -> int:
        return elem_size(dtype)


def _descs(buckets):
    descs = (BucketDesc * max(1, len(buckets)))()
    for i, (dst, srcs, length) in enumerate(buckets):
        if len(srcs) > MAX_SRCS:
            raise ReduceError(EARGS, f"bucket {i}: more than {MAX_SRCS} sources")
        descs[i].dst = _ptr(dst)
        for k, s in enumerate(srcs):
            descs[i].srcs[k] = _ptr(s)
        descs[i].len = int(length)
        descs[i].n = len(srcs)
    return descs


class Plan:
    """``byteps_reduce_plan``: a Prophet block's bucket table resident on the device."""

    def __init__(self, lib, buckets, dtype, mode):
        self.lib = lib
        self.handle = _vp()
        self._keep = buckets          # keep the tensors alive
        self.first = buckets[0][0] if buckets else None
        _check(lib.byteps_reduce_plan_create(_descs(buckets), len(buckets), int(dtype),
                                             int(mode), ctypes.byref(self.handle)))

    def launch(self, stream=None) -> None:
        _check(self.lib.byteps_reduce_plan_launch(self.handle, _stream_of(self.first, stream)))

    def close(self) -> None:
        if self.handle:
            self.lib.byteps_reduce_plan_destroy(self.handle)
            self.handle = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _create_plain(lib, descs, n, wide_dtype, wire_dtype, out):
    """The plain plan's creator: the fp16 wire has an entry of its own."""
    if wire_dtype == DType.FLOAT16:
        return lib.byteps_reduce_cast_plan_create(descs, n, wide_dtype, out)
    return lib.byteps_reduce_cast_plan_create_wire(descs, n, wide_dtype, wire_dtype, out)


# Per scheme of a cast plan: the descriptor, the creator (library, descriptors,
# count, wide dtype, wire dtype, out-pointer), and for a segment's fourth item
# the descriptor's field, its value there and its bounds check (element count,
# item).
_CAST_SCHEMES = {
    "plain": (CastDesc, _create_plain, None, None, None),
    "ef": (CastEfDesc, lambda lib, *a: lib.byteps_reduce_cast_plan_create_ef(*a),
           "resid", _ptr, lambda nelem, resid: _fits(int(nelem) * 4, resid)),
    "sr": (CastSrDesc, lambda lib, *a: lib.byteps_reduce_cast_plan_create_sr(*a),
           "key", lambda key: int(key) & 0xffffffff, None),
}


def _check_scalar_f32(x, name: str, device=None) -> None:
    """``x``: a 1-element float32 device tensor (on ``device`` if given)."""
    import torch
    if not hasattr(x, "data_ptr") or x.dtype != torch.float32 or x.numel() != 1:
        raise ValueError(f"{name} must be a 1-element float32 device tensor, got "
                         f"{getattr(x, 'dtype', type(x))} of "
                         f"{x.numel() if hasattr(x, 'numel') else '?'} elements")
    if x.device.type != "cuda" or (device is not None and x.device != device):
        raise ValueError(f"{name} is on {x.device}, expected {device or 'a device'}")
    _fits(4, x)


class ClipRecord:
    """``byteps_clip_record`` on the device: ``tensor`` is its 32 bytes, and
    ``sumsq``, ``nonfinite``, ``norm`` (float64) and ``coef``, ``mult``
    (float32) are 0-d views of it, valid in stream order after
    ``GpuReducer.clip_record``.  ``mult`` is what
    ``CastPlan.decompress(scale=)`` takes."""

    def __init__(self, device):
        import torch
        self.tensor = torch.zeros(32, dtype=torch.uint8, device=device)
        f64, f32 = self.tensor.view(torch.float64), self.tensor.view(torch.float32)
        self.sumsq, self.nonfinite, self.norm = f64[0], f64[1], f64[2]
        self.coef, self.mult = f32[6], f32[7]
        self._keep = None


class CastPlan:
    """``byteps_reduce_cast_plan``: the segments' tile table resident on the
    device.  ``compress`` writes every fp16 side from its wide side,
    ``decompress`` the other way (dividing by ``divisor`` on the fp16 value),
    each as ONE launch; per segment the bytes are those of
    ``GpuReducer.compress_fp16`` / ``decompress_fp16`` — or, for a plan whose
    ``wire_dtype`` is BFLOAT16, of ``GpuReducer.compress`` / ``decompress``.

    Tensor operands are bounds-checked before the library sees them, and the
    plan holds a reference to every one: the device table carries raw
    addresses, and a write through a freed one would be a GPU fault rather
    than an exception.  Raw pointers carry no size and stay the caller's.

    Segments of four, ``(wide, half, nelem, resid)``, make an error-feedback
    plan: ``compress`` writes per segment the bytes of
    ``GpuReducer.compress_ef``, wire and residual; ``decompress`` is the
    plain one and leaves the residuals alone.  The residual tensors are held
    like the others.

    Segments ``(wide, half, nelem, SrKey(key))`` make a stochastic-rounding
    plan: ``compress(step=s)`` writes per segment the bytes of
    ``GpuReducer.compress_sr(..., key, s, ...)``, a ``compress`` without a
    step is refused (EARGS), and ``decompress`` is the plain one."""

    def __init__(self, lib, segments, wide_dtype, wire_dtype=DType.FLOAT16):
        self.lib = lib
        self.wire_dtype = int(wire_dtype)
        self.handle = _vp()
        segments = [tuple(s) for s in segments]
        keyed = [len(s) == 4 and isinstance(s[3], SrKey) for s in segments]
        self.stochastic = any(keyed)
        self.error_feedback = not self.stochastic and any(len(s) == 4 for s in segments)
        if self.stochastic and not all(keyed):
            raise ValueError("cast plan: every segment carries a key, or none does")
        if self.error_feedback and not all(len(s) == 4 for s in segments):
            raise ValueError("cast plan: every segment carries a residual, or none does")
        desc, create, field, value, fits = _CAST_SCHEMES[
            "sr" if self.stochastic else "ef" if self.error_feedback else "plain"]
        for s in segments:
            if len(s) != (3 if field is None else 4):
                raise ValueError(f"cast plan: a segment of {len(s)} items")
            _fits_cast(s[2], s[1], s[0], wide_dtype)
            if fits is not None:
                fits(s[2], s[3])
        self._keep = segments         # keep the tensors alive, the residuals too
        self.first = next((s[0] for s in segments if hasattr(s[0], "device")), None)
        self.nsegs = len(segments)
        descs = (desc * max(1, len(segments)))()
        for d, s in zip(descs, segments):
            d.wide, d.half, d.nelem = _ptr(s[0]), _ptr(s[1]), int(s[2])
            if field is not None:
                setattr(d, field, value(s[3]))
        _check(create(lib, descs, len(segments), int(wide_dtype), self.wire_dtype,
                      ctypes.byref(self.handle)))

    def compress(self, stream=None, *, step: int | None = None) -> None:
        """One launch; ``step`` (mod 2^32) for a stochastic-rounding plan and
        for no other."""
        if step is not None:
            _check(self.lib.byteps_reduce_cast_plan_compress_sr(self.handle,
                                                                int(step) & 0xffffffff,
                                                                _stream_of(self.first, stream)))
            return
        _check(self.lib.byteps_reduce_cast_plan_compress(self.handle,
                                                         _stream_of(self.first, stream)))

    def _check_stats(self, stats) -> None:
        """A statistics tensor is float64, contiguous, of ``2 * nsegs``
        elements, on the plan's device."""
        if hasattr(stats, "data_ptr"):
            import torch
            if stats.dtype != torch.float64:
                raise ValueError(f"stats must be float64, got {stats.dtype}")
            if not stats.is_contiguous():
                raise ValueError("stats must be contiguous")
            if stats.numel() != 2 * self.nsegs:
                raise ValueError(f"stats has {stats.numel()} elements, the plan's "
                                 f"{self.nsegs} segments need {2 * self.nsegs}")
            dev = getattr(self.first, "device", None)
            if stats.device.type != "cuda" or (dev is not None and stats.device != dev):
                raise ValueError(f"stats is on {stats.device}, the plan on {dev or 'a device'}")
            _fits(16 * self.nsegs, stats)

    def measure(self, divisor: int = 1, stream=None, stats=None) -> None:
        """The statistics of ``decompress(divisor, stats=stats)`` — the same
        rows, bit for bit — without the decompress: the 2-byte sides are read
        and no wide side is written (byteps_reduce_cast_plan_measure).
        ``stats`` as for ``decompress``."""
        if stats is None:
            raise ValueError("measure needs a stats tensor")
        self._check_stats(stats)
        self._stats = stats           # held: the launches are asynchronous
        _check(self.lib.byteps_reduce_cast_plan_measure(
            self.handle, int(divisor), _ptr(stats), _stream_of(self.first, stream)))

    def decompress(self, divisor: int = 1, stream=None, stats=None, scale=None) -> None:
        """One launch.  With ``scale`` — a 1-element float32 device tensor,
        typically a :class:`ClipRecord`'s ``mult`` — every value written is
        multiplied by it, rounded once to the wide dtype
        (byteps_reduce_cast_plan_decompress_scaled); the plan holds the tensor
        until its next scaled launch or ``close``.  ``scale`` excludes
        ``stats``.  With ``stats`` — a contiguous float64 device tensor
        of ``2 * nsegs`` elements on the plan's device, or a raw pointer to as
        much — the same bytes are written and ``stats[2 s], stats[2 s + 1]``
        receive segment ``s``'s sum of the squares of the finite values
        written (f64) and the count of the non-finite ones
        (byteps_reduce_cast_plan_decompress_stats; a second, small launch on
        the same stream).  A tensor is bounds-checked like the other
        operands, and the plan holds it until its next statistics call or
        ``close``: the launches are asynchronous.  A plan's first statistics
        call allocates its partial sums; two statistics launches of one plan
        must not run concurrently."""
        if stats is not None and scale is not None:
            raise ValueError("decompress: stats and scale exclude each other "
                             "(measure, then decompress(scale=))")
        if scale is not None:
            if hasattr(scale, "data_ptr"):
                _check_scalar_f32(scale, "scale", getattr(self.first, "device", None))
            self._scale = scale       # held: the launch is asynchronous
            _check(self.lib.byteps_reduce_cast_plan_decompress_scaled(
                self.handle, int(divisor), _ptr(scale), _stream_of(self.first, stream)))
            return
        if stats is None:
            _check(self.lib.byteps_reduce_cast_plan_decompress(self.handle, int(divisor),
                                                               _stream_of(self.first, stream)))
            return
        self._check_stats(stats)
        self._stats = stats           # held: the launches are asynchronous
        _check(self.lib.byteps_reduce_cast_plan_decompress_stats(
            self.handle, int(divisor), _ptr(stats), _stream_of(self.first, stream)))

    def close(self) -> None:
        if self.handle:
            self.lib.byteps_reduce_cast_plan_destroy(self.handle)
            self.handle = _vp()
        self._keep = []
        self._stats = None
        self._scale = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class SgdPlan:
    """An SGD plan (``byteps_reduce_cast_plan_create_sgd``): per segment the
    float32 parameter, the 2-byte wire buffer and the float32 momentum buffer.
    ``apply`` is one launch; per element the arithmetic is
    ``prophet_amd.sgd.sgd_step``'s, bit for bit.  Tensor operands are
    bounds-checked before the library sees them and held until ``close``, as
    a :class:`CastPlan` holds its own.  The library refuses every other cast
    plan call on this plan: a decompress would write gradients over the
    parameters."""

    def __init__(self, lib, segments, wire_dtype=DType.FLOAT16):
        self.lib = lib
        self.wire_dtype = int(wire_dtype)
        self.handle = _vp()
        segments = [tuple(s) for s in segments]
        for s in segments:
            if len(s) != 4:
                raise ValueError(f"sgd plan: a segment of {len(s)} items")
            _fits_cast(s[2], s[1], s[0], DType.FLOAT32)
            _fits(int(s[2]) * 4, s[3])
        self._keep = segments         # keep the tensors alive, the momenta too
        self._rec = None
        self.first = next((s[0] for s in segments if hasattr(s[0], "device")), None)
        self.nsegs = len(segments)
        descs = (CastSgdDesc * max(1, len(segments)))()
        for d, s in zip(descs, segments):
            d.param, d.half, d.nelem, d.momentum = _ptr(s[0]), _ptr(s[1]), int(s[2]), _ptr(s[3])
        _check(lib.byteps_reduce_cast_plan_create_sgd(descs, len(segments), self.wire_dtype,
                                                      ctypes.byref(self.handle)))

    def apply(self, divisor: int = 1, *, lr: float, momentum: float = 0.0,
              weight_decay: float = 0.0, nesterov: bool = False, record=None,
              skip_nonfinite: bool = False, stream=None) -> None:
        """One launch (byteps_reduce_cast_plan_apply_sgd).  ``record``: a
        :class:`ClipRecord` on the plan's device (or a raw pointer to one),
        whose ``mult`` scales the gradient; with ``skip_nonfinite`` a record
        whose ``nonfinite`` is not 0 leaves every parameter and momentum byte
        as it was, decided on the device.  The plan holds the record until its
        next launch or ``close``."""
        rec = record
        if isinstance(record, ClipRecord):
            dev = getattr(self.first, "device", None)
            if dev is not None and record.tensor.device != dev:
                raise ValueError(f"record is on {record.tensor.device}, the plan on {dev}")
            _fits(32, record.tensor)
            rec = record.tensor
        elif record is not None and not isinstance(record, int):
            raise ValueError(f"record must be a ClipRecord, got {type(record)!r}")
        self._rec = record            # held: the launch is asynchronous
        h = SgdHyper(float(lr), float(momentum), float(weight_decay), 1 if nesterov else 0)
        _check(self.lib.byteps_reduce_cast_plan_apply_sgd(
            self.handle, int(divisor), ctypes.byref(h), _ptr(rec), 1 if skip_nonfinite else 0,
            _stream_of(self.first, stream)))

    def close(self) -> None:
        if self.handle:
            self.lib.byteps_reduce_cast_plan_destroy(self.handle)
            self.handle = _vp()
        self._keep = []
        self._rec = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BlockQueue:
    """``byteps_reduce_blockq``: a persistent consumer over an iteration's blocks.

    Per iteration: ``launch()`` once and ``release(b)`` for every block, in
    either order (epochs pair the k-th launch with the k-th release of each
    block; a block is consumed once it and all earlier blocks are released),
    ``status()`` to learn whether the launch gave up waiting."""

    def __init__(self, lib, blocks, dtype, mode):
        self.lib = lib
        self.handle = _vp()
        buckets = [b for blk in blocks for b in blk]
        ends, acc = [], 0
        for blk in blocks:
            acc += len(blk)
            ends.append(acc)
        self.nblocks = len(blocks)
        self._keep = buckets
        self.first = buckets[0][0] if buckets else None
        arr = (_int * max(1, len(ends)))(*ends)
        _check(lib.byteps_reduce_blockq_create(_descs(buckets), len(buckets), arr, len(ends),
                                               int(dtype), int(mode),
                                               ctypes.byref(self.handle)))

    def config(self, wg_per_cu: int = -1, timeout_s: float = 0.0) -> None:
        """``wg_per_cu`` 0: dispatch-ordered consumer (default); 1..8:
        persistent workgroups per CU; < 0 keeps.  ``timeout_s`` <= 0 keeps."""
        _check(self.lib.byteps_reduce_blockq_config(self.handle, int(wg_per_cu),
                                                    float(timeout_s)))

    def launch(self, stream=None) -> None:
        _check(self.lib.byteps_reduce_blockq_launch(self.handle, _stream_of(self.first, stream)))

    def release(self, block: int = -1, stream=None) -> None:
        _check(self.lib.byteps_reduce_blockq_release(self.handle, int(block),
                                                     _stream_of(self.first, stream)))

    def release_range(self, first: int, count: int, stream=None) -> None:
        """Release blocks [first, first + count) with one kernel."""
        _check(self.lib.byteps_reduce_blockq_release_range(self.handle, int(first), int(count),
                                                           _stream_of(self.first, stream)))

    def host_releases(self, on: bool = True) -> None:
        """Later launches carry a helper workgroup that forwards host
        releases (``release_host``); dispatch-ordered consumer only."""
        _check(self.lib.byteps_reduce_blockq_host_releases(self.handle, 1 if on else 0))

    def release_host(self, first: int, count: int = 1) -> None:
        """Release blocks [first, first + count) from the host: no stream, no
        kernel.  Their data must already be complete and visible to the device."""
        _check(self.lib.byteps_reduce_blockq_release_host(self.handle, int(first), int(count)))

    def overlap(self, on: bool = True) -> None:
        """Consecutive launches may overlap (byteps_reduce_blockq_overlap):
        a launch no longer orders its stream after the fold — ``join``
        before reading the outputs or rewriting the inputs."""
        _check(self.lib.byteps_reduce_blockq_overlap(self.handle, 1 if on else 0))

    def join(self, stream=None) -> None:
        """``stream`` (default: torch's current stream) waits on the device
        for every block-queue launch of the device so far."""
        _check(self.lib.byteps_reduce_blockq_join(self.handle, _stream_of(self.first, stream)))

    def status(self, stream=None) -> None:
        _check(self.lib.byteps_reduce_blockq_status(self.handle, _stream_of(self.first, stream)))

    def stream(self):
        """The device's consumer stream (byteps_reduce_blockq_stream) as a
        torch ExternalStream: launch here to skip the fork/join onto it."""
        import torch
        p = _vp()
        _check(self.lib.byteps_reduce_blockq_stream(self.handle, ctypes.byref(p)))
        return torch.cuda.ExternalStream(p.value)

    def release_stream(self):
        """The device's release stream (byteps_reduce_blockq_release_stream) as
        a torch ExternalStream: a hardware queue on a compute pipe no consumer
        queue uses — queue pushes and stream releases here."""
        import torch
        p = _vp()
        _check(self.lib.byteps_reduce_blockq_release_stream(self.handle, ctypes.byref(p)))
        return torch.cuda.ExternalStream(p.value)

    def queue_ids(self) -> dict:
        """HSA queue ids of the device's consumer queues and release queue
        (byteps_reduce_blockq_queue_ids; 0 = not made yet)."""
        ids = (ctypes.c_uint64 * 4)()
        n = self.lib.byteps_reduce_blockq_queue_ids(self.handle, ids, 4)
        if n < 0:
            _check(n)
        return {"consumer": [ids[0], ids[1], ids[2]], "release": ids[3]}

    def debug(self) -> dict:
        """byteps_reduce_blockq_debug (synchronises the device)."""
        nb = self.nblocks
        buf = (ctypes.c_uint32 * (4 + 3 * nb + 8))()
        k = self.lib.byteps_reduce_blockq_debug(self.handle, buf, len(buf))
        if k < 0:
            _check(k)
        v = list(buf[:k])
        return {"launch_epoch": v[0], "nblocks": v[1], "err": v[2],
                "rel_epoch": v[3:3 + nb], "words": v[3 + nb:3 + 2 * nb],
                "block_first": v[3 + 2 * nb:4 + 3 * nb], "table_intact": bool(v[-1])}

    def close(self) -> None:
        if self.handle:
            self.lib.byteps_reduce_blockq_destroy(self.handle)
            self.handle = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# torch-tensor convenience: whole-tensor ops with dtype taken from the tensor
def tensor_sum_n(dst, srcs, mode: int = MODE_REFERENCE, reducer: GpuReducer | None = None):
    from .dtypes import from_torch
    r = reducer or GpuReducer()
    nbytes = dst.numel() * dst.element_size()
    for s in srcs:
        if s.numel() * s.element_size() != nbytes or s.dtype != dst.dtype:
            raise ReduceError(EARGS, "sources must match dst in dtype and size")
        if not s.is_contiguous():
            raise ReduceError(EARGS, "sources must be contiguous")
    if not dst.is_contiguous():
        raise ReduceError(EARGS, "dst must be contiguous")
    r.sum_n(dst, srcs, nbytes, from_torch(dst.dtype), mode)
    return dst
