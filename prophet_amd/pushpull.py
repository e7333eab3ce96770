"""End-to-end push_pull of whole gradient tensors over the GPU-resident PS server.

The worker side of byteps/common/operations.cc and the server side of
byteps/server/server.cc, with an in-process transport:

* ``declare`` — every worker registers its tensors in the same order; the
  position is the tensor's declared key (BytePSGlobal's declared-tensor list);
* ``init_tensor`` — ``InitTensor`` (operations.cc:219-316): the key list is
  ``(declared_key << 16) + i`` for the partitions of ``size`` bytes under the
  partition bound (global.cc:128-135, aligned down to 8 * local_size), and
  each partition is pushed once, blocking — the store's init round and the
  workers' global barrier (operations.cc:301-302);
* ``push_pull`` — ``EnqueueTensor`` (operations.cc:138-217) with
  ``PartitionTensor`` (:99-136): the tensor is cut into the same partitions,
  each one is pushed under its key and pulled back, and the aggregate lands at
  its offset of the output — optionally in the order the Prophet PUSH
  scheduler releases partitions (scheduled_queue.cc:217-296,
  ``prophet_amd.prophet.ProphetPushQueue``);
* ``push_pull(average=True)``, ``push_pull_async`` / ``poll`` /
  ``synchronize`` and ``broadcast`` (push_pull with zeros on the non-root
  ranks) — the byteps/torch API shapes (ops.py, __init__.py:244-272);
* the server front end decodes the request word like ``BytePSHandler``
  (``DepairDataHandleType``, server.h:77-88, of ``GetCommandType``'s Cantor
  pairing, common.cc:99-102) and hands the bytes to ``PSServer``.

Buffers may be host (numpy / CPU tensors) or device tensors; every byte of
arithmetic is the server's HIP fold.

``init_tensor(..., compression=Compression.fp16)`` (or ``Compression.bf16``,
read bf16 for fp16 below) makes a floating tensor
travel as fp16 (byteps/torch/__init__.py:133-170): the context's size, dtype
and partitions are those of the COMPRESSED tensor, every call casts into a
per-context fp16 staging buffer, pushes and pulls that, and one fused launch
widens the result into the output — dividing the fp16 value first when
``average=True``, as the reference's callback does on the compressed tensor
(byteps/torch/ops.cc:77-81).  DESIGN.md §11 has the stream-ordering argument.

``push_pull_iteration`` casts all its compressed device tensors at once: one
cast-plan launch before the first push and one after the last pull
(``FP16Compressor.compress_many_into`` / ``decompress_many_into``), with the
plans kept on the worker between iterations.

``Compression.fp16_ef`` / ``Compression.bf16_ef`` (float32 tensors) keep a
zeroed f32 residual beside the staging buffer: every push_pull casts
``tensor + residual`` and leaves the rounding error in the residual
(``compress_ef_into``; in ``push_pull_iteration`` one error-feedback plan
launch).  The init push is the plain cast and leaves the residual zero; the
decompress, and so ``average=``, is the plain compressor's.
``Worker.residual`` / ``reset_residual`` read and zero it.

``Compression.fp16_sr`` / ``Compression.bf16_sr`` (float32 tensors) round
stochastically and keep no state beside a counter: a context's key is ``x0`` of
Philox2x32-10(declared key, rank, ``Worker(sr_seed=...)``) — ranks draw
independent bits — and the step is a per-worker counter (``Worker.sr_step``)
that advances by one for every stochastic compress call or plan launch, so no
``(key, step)`` pair is used twice.  The init push is the plain cast; the
decompress is the plain compressor's.

``push_pull(..., stats=True)`` / ``push_pull_iteration(..., stats=True)`` make
the decompress the statistics one (``decompress_many_into(..., stats=)``,
DESIGN.md §11.5) and leave ``Worker.grad_stats``: per compressed context the
sum of squares and the non-finite count of the aggregate just written — the
global gradient norm and GradScaler's ``found_inf`` without a second sweep.
For device tensors the rows and everything derived from them stay on the
device, in stream order.

``push_pull_iteration(..., clip_norm=, clip_eps=, unscale=)`` clips the whole
iteration's gradients by their global norm and unscales them inside the
decompress: after the last pull every compressor group is
measured into one rows tensor, one clip record is made over all rows, and
every group is decompressed times the record's ``mult``.  It leaves
``Worker.grad_clip`` (:class:`GradClip`) and ``Worker.grad_stats``.

``push_pull_iteration(..., apply=SgdStep(params, lr, ...))`` ends the
iteration in the parameters instead: after the last pull
every compressor group runs ``apply_sgd_many`` — one launch per device that
reads the pulled wire aggregate, the parameter and the context's momentum
buffer and updates the last two in place — and the gradients in ``tensors``
are not written at all.  With ``clip_norm`` the groups are measured and the
one clip record made as above, and the step multiplies by its ``mult``; with
``SgdStep(skip_nonfinite=True)`` an overflowed iteration leaves parameters
and momenta untouched, decided on the device.  ``Worker.momentum`` /
``reset_momentum`` read and zero a context's momentum buffer.
"""
from __future__ import annotations

import threading
from dataclasses import dataclass, field

from .buckets import (DEFAULT_PARTITION_BYTES, cantor_command, depair_command,
                      local_size_from_env, partition_bound, partition_bytes_from_env)
from .compression import CastPlanCache, Compression
from .dtypes import DType, elem_size
from .reducer import SrKey

K_DEFAULT_PUSH_PULL = 0     # RequestType::kDefaultPushPull (common.h:68-71)


class ServerFrontend:
    """The handler in front of the GPU-resident server: decodes the request
    word, checks one key per request (server.cc:150-171) and forwards."""

    def __init__(self, server, size: int | None = None):
        self.server = server
        cfg = getattr(server, "cfg", None)
        self.size = size if size is not None else (cfg.num_workers if cfg is not None else None)

    def push(self, cmd: int, key: int, worker: int, data, nbytes: int) -> None:
        req, dtype = depair_command(cmd)
        if req != K_DEFAULT_PUSH_PULL:       # server.cc:151 CHECK_EQ(type.requestType, ...)
            raise ValueError(f"request type {req} is not kDefaultPushPull")
        self.server.push(key, worker, data, dtype, nbytes=nbytes)

    def pull(self, key: int, out, nbytes: int) -> None:
        self.server.pull(key, out, nbytes=nbytes)


@dataclass
class Context:
    """BPSContext (common.h): one declared tensor's keys and partitions."""
    name: str
    declared_key: int
    size: int = 0
    dtype: int = 0
    key_list: list = field(default_factory=list)
    parts: list = field(default_factory=list)      # (key, offset, len) in bytes
    initialized: bool = False
    # compression (None: the tensor travels as it is): the compressor, the
    # caller's dtype and byte size, and the buffer of the compressor's wire
    # dtype (fp16 or bf16) that is pushed from and pulled into; size / dtype / parts above are the compressed ones
    compressor: object = None
    orig_dtype: int = 0
    orig_size: int = 0
    staging: object = None
    # the compressor's per-tensor operand of a cast, as cast plans take it:
    # error feedback (Compression.*_ef) — the f32 residual, of the tensor's
    # kind, device and element count; stochastic rounding (Compression.*_sr) —
    # the context's Philox key, an SrKey; None otherwise
    extra: object = None
    # push_pull_iteration(apply=SgdStep): the f32 momentum buffer, zeroed on
    # first use where the parameter lives; None before
    momentum: object = None
    init_lock: threading.Lock = field(default_factory=threading.Lock)

    @property
    def residual(self):
        """The error-feedback residual, or None."""
        return None if isinstance(self.extra, SrKey) else self.extra

    @property
    def sr_key(self) -> int:
        """The stochastic-rounding key, or 0."""
        return int(self.extra) if isinstance(self.extra, SrKey) else 0


class GradStats:
    """The decompress statistics of one ``push_pull(stats=True)`` /
    ``push_pull_iteration(stats=True)``: ``names`` — the compressed contexts,
    in row order; ``rows`` — float64 ``[len(names), 2]``, row i the sum of the
    squares of the finite values written to context i's output and the count
    of its non-finite ones (``compression.decompress_stats``); ``skipped`` —
    the contexts of the call that travel uncompressed and so have no row.
    ``rows`` lives where the outputs live.  For device rows every method
    returns a 0-d device tensor and nothing synchronises with the host: a
    caller can skip (``torch.where(stats.nonfinite() > 0, ...)``) on the device
    in stream order.  To clip by the global norm, do not multiply the
    gradients afterwards: ``push_pull_iteration(clip_norm=...)`` clips (and
    unscales) inside the decompress, which writes them anyway
    (:class:`GradClip`)."""

    def __init__(self, names, rows, skipped=()):
        self.names = list(names)
        self.rows = rows
        self.skipped = list(skipped)

    def __getitem__(self, name: str):
        """The row of context ``name``: ``(sumsq, nonfinite)``."""
        return self.rows[self.names.index(name)]

    def sumsq(self):
        """The sum of squares over all rows."""
        return self.rows[:, 0].sum()

    def nonfinite(self):
        """The number of non-finite values over all rows (float64)."""
        return self.rows[:, 1].sum()

    def norm(self):
        """The global L2 norm of the finite values: ``sqrt(sumsq())``."""
        t = self.sumsq()
        return t.sqrt() if hasattr(t, "data_ptr") else t ** 0.5


class GradClip:
    """The clip record of one ``push_pull_iteration(clip_norm=...)``:
    ``norm`` — the L2 norm of the unscaled aggregate over its finite values
    (float64); ``coef`` — ``min(1, clip_norm / (norm + eps))`` and ``mult`` —
    ``coef * unscale``, what every floating output was multiplied by
    (float32); ``found_inf`` — the number of non-finite values (float64: skip
    the step if it is not 0); ``sumsq`` — the sum of squares before the
    unscale.  ``names`` / ``rows`` — the floating contexts and their
    statistics rows BEFORE the clip, the compressed ones first (as
    ``grad_stats``), then the uncompressed; ``skipped`` — the integer
    contexts, which are left alone.  For device tensors every field is a 0-d
    device tensor (views of ``record``, a ``reducer.ClipRecord``) and nothing
    synchronises with the host."""

    def __init__(self, record, names, rows, skipped=()):
        self.record = record
        self.norm, self.coef, self.mult = record.norm, record.coef, record.mult
        self.found_inf, self.sumsq = record.nonfinite, record.sumsq
        self.names = list(names)
        self.rows = rows
        self.skipped = list(skipped)


@dataclass
class SgdStep:
    """``push_pull_iteration(apply=...)``: SGD with momentum and weight decay
    as the end of the iteration (``prophet_amd.sgd`` is the arithmetic).
    ``params`` maps every floating context's name to its float32 parameter,
    of the gradient's size and in the gradient's place; it is updated in
    place.  ``skip_nonfinite`` (with ``clip_norm``): an iteration whose
    aggregate holds a non-finite value leaves parameters and momenta as they
    were."""
    params: dict
    lr: float
    momentum: float = 0.0
    weight_decay: float = 0.0
    nesterov: bool = False
    skip_nonfinite: bool = False


def _finite_row(row, x) -> None:
    """``row[:] = (sum of squares of the finite values of x in float64, count
    of the others)``: the decompress statistics' definition, for a tensor that
    travels uncompressed; on x's device, in stream order."""
    if hasattr(x, "data_ptr"):
        import torch
        v = x.detach().reshape(-1).to(torch.float64)
        fin = torch.isfinite(v)
        row[0] = torch.where(fin, v * v, torch.zeros_like(v)).sum()
        row[1] = (~fin).sum().to(torch.float64)
        return
    from .compression import decompress_stats
    row[0], row[1] = decompress_stats(x)


def _scale_(x, mult) -> None:
    """In-place ``x *= mult`` (float32; a 0-d device tensor for a device x)
    with one rounding: the f32 product for f32 and the 2-byte types, the f64
    product for f64."""
    if hasattr(x, "data_ptr") and x.device.type == "cuda":
        import torch
        if x.dtype == torch.float64:
            x.mul_(mult.to(torch.float64))
        elif x.dtype == torch.float32:
            x.mul_(mult)
        else:
            x.copy_((x.to(torch.float32) * mult).to(x.dtype))
        return
    from .compression import _scale_host_
    _scale_host_(x, mult)


def _place(x):
    """The device of a device tensor, None for the host."""
    dev = getattr(x, "device", None) if hasattr(x, "data_ptr") else None
    return dev if dev is not None and dev.type == "cuda" else None


def _is_float(x) -> bool:
    if hasattr(x, "data_ptr"):
        return bool(x.is_floating_point())
    import numpy as np
    return bool(np.issubdtype(x.dtype, np.floating))


def _stat_rows(n: int, like):
    """float64 ``[n, 2]`` where ``like`` lives."""
    if hasattr(like, "data_ptr"):
        import torch
        return torch.empty((n, 2), dtype=torch.float64, device=like.device)
    import numpy as np
    return np.empty((n, 2), dtype=np.float64)


class Worker:
    """One BytePS worker (its root device) talking to the server front end."""

    def __init__(self, rank: int, frontend: ServerFrontend,
                 partition_bytes: int | None = None, local_size: int | None = None, *,
                 sr_seed: int = 0):
        """``partition_bytes`` / ``local_size`` default to the reference's
        environment: BYTEPS_PARTITION_BYTES (global.cc:128-130, else 4,096,000)
        and BYTEPS_LOCAL_SIZE (communicator.cc:71-77, else 1); the bound is
        AlignTo(partition_bytes, 8 * local_size), rounded down (global.cc:135).
        ``sr_seed``: the seed of this job's stochastic rounding
        (``Compression.*_sr``); the same on every worker."""
        self.rank = rank
        self.frontend = frontend
        if partition_bytes is None:
            partition_bytes = partition_bytes_from_env()
        if local_size is None:
            local_size = local_size_from_env()
        if local_size < 1:
            raise ValueError("local_size must be >= 1")
        self.bound = partition_bound(partition_bytes, local_size)
        if self.bound <= 0:
            raise ValueError(f"partition bound must be positive (BYTEPS_PARTITION_BYTES="
                             f"{partition_bytes}, local_size={local_size})")
        self.contexts: dict[str, Context] = {}
        self._declared: list[str] = []
        self._pool = None
        self._handles: dict[int, tuple] = {}
        self._next_handle = 0
        # push_pull_iteration's cast plans: found again by every segment's
        # (tensor address, staging address, element count), at most 8 (an
        # iteration that mixes the six casting compressors uses six), the
        # least recently used destroyed first
        self._cast_plans = CastPlanCache(8)
        # stochastic rounding: the seed the contexts' keys derive from, and
        # the step counter — one per compress call or plan launch, under a
        # lock (push_pull_async runs on the worker's own thread)
        self.sr_seed = int(sr_seed) & 0xffffffff
        self._sr_step = 0
        self._sr_lock = threading.Lock()
        # the decompress statistics of the last push_pull / push_pull_iteration
        # with stats=True (GradStats); None before the first
        self.grad_stats = None
        # the clip record of the last push_pull_iteration with clip_norm
        # (GradClip); None before the first
        self.grad_clip = None

    @property
    def sr_step(self) -> int:
        """Stochastic compress calls and plan launches so far: the step the
        next one rounds under."""
        return self._sr_step

    def _next_step(self, compressor):
        """The step the next compress of ``compressor`` rounds under: drawn
        for stochastic rounding alone, None for every other."""
        if not compressor.STOCHASTIC:
            return None
        with self._sr_lock:
            step = self._sr_step
            self._sr_step += 1
        return step

    # ------------------------------------------------------------ declare/init
    def declare(self, name: str) -> int:
        """Register a tensor; its position is its declared key."""
        if name not in self.contexts:
            self.contexts[name] = Context(name, len(self._declared))
            self._declared.append(name)
        return self.contexts[name].declared_key

    def _partition(self, size: int):
        """PartitionTensor (operations.cc:99-136): [offset, len) under the bound."""
        out, acc = [], 0
        while acc < size:
            ln = min(self.bound, size - acc)
            out.append((acc, ln))
            acc += ln
        return out

    def init_tensor(self, name: str, data, dtype: int, compression=Compression.none) -> Context:
        """InitTensor (operations.cc:219-316): keys, then one blocking init push
        per partition (every worker's init push of a key returns only once all
        of them arrived: the global barrier).  ``compression``: how the tensor
        travels from now on (``Compression.fp16``: floating tensors as fp16,
        ``Compression.bf16``: as bf16 — the keys, partitions and request dtype
        are the compressed tensor's; integers and tensors already of the wire
        dtype pass through as with ``Compression.none``)."""
        self.declare(name)
        ctx = self.contexts[name]
        size = _nbytes(data)
        with ctx.init_lock:
            if ctx.initialized:
                return ctx
            if size <= 0:
                raise ValueError("init tensor size not larger than 0")      # operations.cc:229
            if compression.compresses(data):
                ctx.compressor = compression
                ctx.orig_dtype, ctx.orig_size = int(dtype), size
                ctx.staging = compression.wire_like(data)
                from .sr import context_key
                ctx.extra = compression.cast_extra(
                    data, lambda: context_key(ctx.declared_key, self.rank, self.sr_seed))
                # the init push is the plain cast: the residual stays zero
                data = compression.compress_into(ctx.staging, data)
                size, dtype = _nbytes(data), DType(compression.WIRE_DTYPE)
            ctx.size, ctx.dtype = size, int(dtype)
            start = ctx.declared_key << 16
            ctx.parts = [(start + i, off, ln) for i, (off, ln) in enumerate(self._partition(size))]
            ctx.key_list = [k for k, _, _ in ctx.parts]
            assert len(ctx.key_list) == (size + self.bound - 1) // self.bound   # :257-259
            cmd = cantor_command(K_DEFAULT_PUSH_PULL, ctx.dtype)
            for key, off, ln in ctx.parts:
                self.frontend.push(cmd, key, self.rank, _slice(data, off, ln), ln)
            ctx.initialized = True
        return ctx

    # ---------------------------------------------------------------- push_pull
    def push_pull(self, name: str, tensor, output=None, order=None,
                  average: bool = False, stats: bool = False) -> None:
        """EnqueueTensor + the PUSH/PULL stages for one tensor: push every
        partition (in ``order`` — a list of partition indices — if given), then
        pull every partition into ``output`` (default: ``tensor`` itself, in
        place, as byteps_push_pull does).  ``average``: divide the sum by the
        number of workers afterwards, as byteps/torch's push_pull(average=True)
        does (floating dtypes only).  ``stats``: a compressed context's
        decompress also leaves ``grad_stats`` (one row; a device tensor's
        through a one-segment cast plan kept on this worker); an uncompressed
        context has no row and is named in ``grad_stats.skipped``."""
        ctx = self.contexts[name]
        if not ctx.initialized:
            raise RuntimeError(f"{name}: init_tensor first")
        if ctx.compressor is not None:
            return self._push_pull_compressed(ctx, tensor, output, order, average, stats)
        if stats:
            self.grad_stats = GradStats([], _stat_rows(0, tensor), [name])
        if _nbytes(tensor) != ctx.size:
            raise ValueError(f"{name}: {_nbytes(tensor)} bytes, declared {ctx.size}")
        out = tensor if output is None else output
        if _nbytes(out) != ctx.size:
            raise ValueError(f"{name}: output tensor size does not match")   # operations.cc:151
        cmd = cantor_command(K_DEFAULT_PUSH_PULL, ctx.dtype)
        idx = range(len(ctx.parts)) if order is None else order
        for i in idx:
            key, off, ln = ctx.parts[i]
            self.frontend.push(cmd, key, self.rank, _slice(tensor, off, ln), ln)
        for key, off, ln in ctx.parts:
            self.frontend.pull(key, _slice(out, off, ln), ln)
        if average:
            size = getattr(self.frontend, "size", None)
            if not size:
                raise ValueError("average: the frontend does not know the worker count")
            _divide_(out, size)

    def _push_pull_compressed(self, ctx: Context, tensor, output, order, average: bool,
                              stats: bool = False) -> None:
        """push_pull of a context initialised with a compressor: cast into the
        context's staging buffer, push and pull THAT (its partitions, the wire
        dtype — FLOAT16 or BFLOAT16 — in the request word), then one launch
        widens it into the output, dividing the 2-byte value by the worker
        count first for ``average``.
        Device tensors: both casts run on the calling thread's current stream;
        the output is complete in that stream's order."""
        out = tensor if output is None else output
        for x, what in ((tensor, "tensor"), (out, "output tensor")):
            if _nbytes(x) != ctx.orig_size:
                raise ValueError(f"{ctx.name}: {what} of {_nbytes(x)} bytes, "
                                 f"declared {ctx.orig_size}")
            if x.dtype != tensor.dtype or not ctx.compressor.compresses(x):
                raise ValueError(f"{ctx.name}: {what} dtype {x.dtype} does not match "
                                 "the compressed context")
        divisor = 1
        if average:
            divisor = getattr(self.frontend, "size", None)
            if not divisor:
                raise ValueError("average: the frontend does not know the worker count")
        wire = ctx.compressor.compress_with(ctx.staging, _contiguous(tensor), ctx.extra,
                                            self._next_step(ctx.compressor))
        cmd = cantor_command(K_DEFAULT_PUSH_PULL, ctx.dtype)
        idx = range(len(ctx.parts)) if order is None else order
        for i in idx:
            key, off, ln = ctx.parts[i]
            self.frontend.push(cmd, key, self.rank, _slice(wire, off, ln), ln)
        for key, off, ln in ctx.parts:
            self.frontend.pull(key, _slice(wire, off, ln), ln)
        if not stats:
            ctx.compressor.decompress_into(_contiguous(out), wire, divisor)
            return
        rows = _stat_rows(1, out)
        ctx.compressor.decompress_into(_contiguous(out), wire, divisor, stats=rows[0],
                                       plans=self._cast_plans)
        self.grad_stats = GradStats([ctx.name], rows)

    # byteps/torch/ops.py: push_pull_async -> handle, poll(handle),
    # synchronize(handle).  Calls run in call order on the worker's own
    # thread (BytePS's loops also take a worker's tensors one after another).
    def push_pull_async(self, name: str, tensor, output=None, average: bool = False) -> int:
        from concurrent.futures import ThreadPoolExecutor
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix=f"bps{self.rank}")
        out = tensor if output is None else output
        fut = self._pool.submit(self.push_pull, name, tensor, out, None, average)
        self._next_handle += 1
        self._handles[self._next_handle] = (fut, out)
        return self._next_handle

    def poll(self, handle: int) -> bool:
        return self._handles[handle][0].done()

    def synchronize(self, handle: int):
        """Wait for the push_pull and return its output (errors re-raised)."""
        fut, out = self._handles.pop(handle)
        fut.result()
        return out

    def close(self) -> None:
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
        self._cast_plans.close()

    def residual(self, name: str):
        """The error-feedback residual of a context initialised with
        ``Compression.fp16_ef`` / ``bf16_ef`` (flat f32, the live buffer), or
        ``None`` for any other context."""
        return self.contexts[name].residual

    def reset_residual(self, name: str) -> None:
        """Zero the residual (after a learning-rate step or a restored
        checkpoint, say); nothing to do for a context without one."""
        r = self.contexts[name].residual
        if r is None:
            return
        if hasattr(r, "data_ptr"):
            r.zero_()
        else:
            r.fill(0)

    def broadcast(self, name: str, tensor, root_rank: int, output=None):
        """Broadcast as BytePS does it (byteps/torch/__init__.py:264-272: "push +
        pull ... the non-root tensors all 0", no averaging): the root pushes its
        tensor, every other rank pushes zeros, everyone pulls the sum into
        ``output`` (a new buffer like ``tensor`` if not given; the source is
        left untouched, as test_mxnet.py:116-158 requires).  The tensor must
        have been through ``init_tensor`` — without compression, error
        feedback and stochastic rounding included: parameters are broadcast
        exactly."""
        if self.contexts[name].compressor is not None:
            raise ValueError(f"{name}: broadcast needs a context without compression")
        src = tensor if self.rank == root_rank else _zeros_like(tensor)
        out = _zeros_like(tensor) if output is None else output
        self.push_pull(name, src, output=out)
        return out

    def push_pull_iteration(self, tensors: dict, scheduler=None, average: bool = False,
                            stats: bool = False, clip_norm=None, clip_eps: float = 1e-6,
                            unscale=None, apply: "SgdStep | None" = None) -> list:
        """One training iteration: every declared tensor, gradients arriving in
        backward order (highest declared index first).  With a Prophet
        ``scheduler`` (``ProphetPushQueue``) the partitions are pushed in the
        groups it releases; then every partition is pulled back in place.
        Compressed contexts are cast together: one ``compress_many_into``
        before the first push and one ``decompress_many_into`` after the last
        pull (device tensors: one cast-plan launch each, the plans cached on
        this worker).  ``average``: divide by the number of workers as
        ``push_pull(average=True)`` does — compressed contexts on the 2-byte
        value inside the decompress, the others in place afterwards.
        ``stats``: the decompress is the statistics one and ``grad_stats``
        holds one row per compressed context, grouped by compressor in the
        order the compressors first appear (``grad_stats.names``); the rows
        live where the first compressed tensor lives.
        ``clip_norm``: clip every floating tensor of the iteration by their
        global L2 norm, and multiply by ``unscale`` (a number, or a 1-element
        float32 device tensor: GradScaler's inverse scale), inside the
        decompress: measure every compressor group, one clip record over all
        rows, then the scaled decompress per group — on the current stream,
        nothing synchronises with the host.  Floating tensors that travel
        uncompressed are divided for ``average`` first, measured by torch
        under the same finite-only definition and multiplied in place;
        integer tensors keep the sum they pulled: they are neither divided
        nor multiplied, and are named in ``grad_clip.skipped``.  Leaves ``grad_clip``
        (:class:`GradClip`) and ``grad_stats`` (the rows before the clip).
        All floating tensors live in one place, a device or the host.
        ``apply`` (:class:`SgdStep`): after the last pull the SGD step runs
        inside the decompress — ``apply_sgd_many`` per compressor group in
        place of the decompress — on ``apply.params`` and the contexts'
        momentum buffers; ``tensors``' floating entries, the gradients, are
        not written.  ``clip_norm`` measures and makes the one record as
        above and the step takes its ``mult`` (and, with
        ``apply.skip_nonfinite``, its skip); ``stats`` without ``clip_norm``
        measures into ``grad_stats``.  Every floating context must be
        compressed, float32 and named in ``apply.params`` by a float32
        parameter of its size and place (``ValueError`` before anything is
        pushed); integer tensors keep the sum they pulled and are named in
        ``grad_stats.skipped`` / ``grad_clip.skipped``.
        Returns the release groups as lists of (declared key, partition)."""
        from .prophet import PushTask, release_groups
        ctxs = [self.contexts[n] for n in self._declared if n in tensors]
        if clip_norm is None and unscale is not None:
            raise ValueError("unscale goes with clip_norm")
        if clip_norm is not None:         # before anything is pushed
            if not clip_norm > 0 or clip_norm != clip_norm or clip_norm == float("inf"):
                raise ValueError(f"clip_norm {clip_norm} is not a finite positive number")
            if not clip_eps >= 0:
                raise ValueError(f"clip_eps {clip_eps} < 0")
            places = {_place(tensors[c.name]) for c in ctxs if _is_float(tensors[c.name])}
            if len(places) > 1:
                raise ValueError("clip_norm: the floating tensors live in one place, "
                                 "a device or the host")
        if apply is not None:             # before anything is pushed
            self._check_apply(ctxs, tensors, apply, clip_norm)
        divisor = 1
        if average:
            divisor = getattr(self.frontend, "size", None)
            if not divisor:
                raise ValueError("average: the frontend does not know the worker count")
        arrivals = []
        for c in sorted(ctxs, key=lambda c: -c.declared_key):
            for i, (key, off, ln) in enumerate(c.parts):
                arrivals.append(PushTask(c.declared_key, i, ln, len(c.parts), key))
        if scheduler is None:
            groups = [arrivals]
        else:
            scheduler.reset()
            groups = release_groups(scheduler, arrivals)
        by_key = {c.declared_key: c for c in ctxs}
        # what travels: the tensor itself, or a compressed context's staging
        # buffer — all of them cast before the first partition is pushed
        wire = {c.name: tensors[c.name] if c.compressor is None else c.staging for c in ctxs}
        casts = {}
        for c in ctxs:
            if c.compressor is not None:
                casts.setdefault(c.compressor, []).append(c)
        for comp, cs in casts.items():
            comp.compress_many_with([c.staging for c in cs],
                                    [_contiguous(tensors[c.name]) for c in cs],
                                    [c.extra for c in cs], self._next_step(comp),
                                    plans=self._cast_plans)
        for g in groups:
            for t in g:
                c = by_key[t.grad]
                key, off, ln = c.parts[t.part]
                self.frontend.push(cantor_command(K_DEFAULT_PUSH_PULL, c.dtype), key, self.rank,
                                   _slice(wire[c.name], off, ln), ln)
        for c in ctxs:
            for key, off, ln in c.parts:
                self.frontend.pull(key, _slice(wire[c.name], off, ln), ln)
        if apply is not None:
            self._apply_iteration(ctxs, casts, tensors, divisor, stats, clip_norm, clip_eps,
                                  unscale, apply)
            return [[(t.grad, t.part) for t in g] for g in groups]
        if clip_norm is not None:
            self._clip_iteration(ctxs, casts, tensors, divisor, average, clip_norm, clip_eps,
                                 unscale)
            return [[(t.grad, t.part) for t in g] for g in groups]
        rows, at = None, 0
        if stats:
            names = [c.name for cs in casts.values() for c in cs]
            rows = _stat_rows(len(names), tensors[names[0]] if names else None)
            self.grad_stats = GradStats(names, rows,
                                        [c.name for c in ctxs if c.compressor is None])
        for comp, cs in casts.items():
            # the plan that compressed decompresses too: named by the same
            # residuals or keys
            comp.decompress_many_with([_contiguous(tensors[c.name]) for c in cs],
                                      [c.staging for c in cs], [c.extra for c in cs], divisor,
                                      plans=self._cast_plans,
                                      stats=rows[at:at + len(cs)] if stats else None)
            at += len(cs)
        if average:
            for c in ctxs:
                if c.compressor is None:
                    _divide_(tensors[c.name], divisor)
        return [[(t.grad, t.part) for t in g] for g in groups]

    def _check_apply(self, ctxs, tensors, apply, clip_norm) -> None:
        """What ``push_pull_iteration(apply=)`` asks of its contexts."""
        from .compression import _is_f32
        from .sgd import check_hyper
        check_hyper(apply.lr, apply.momentum, apply.weight_decay, apply.nesterov)
        if apply.skip_nonfinite and clip_norm is None:
            raise ValueError("apply: skip_nonfinite goes with clip_norm (the clip record "
                             "counts the non-finite values)")
        for c in ctxs:
            g = tensors[c.name]
            if not _is_float(g):
                continue
            if c.compressor is None:
                raise ValueError(f"apply: {c.name} is a floating context that is not compressed")
            if not _is_f32(g):
                raise ValueError(f"apply: {c.name} is {g.dtype}, the step needs float32")
            p = apply.params.get(c.name)
            if p is None:
                raise ValueError(f"apply: no parameter for {c.name}")
            if not _is_f32(p) or _nbytes(p) != _nbytes(g) or _place(p) != _place(g) or \
                    hasattr(p, "data_ptr") != hasattr(g, "data_ptr"):
                raise ValueError(f"apply: the parameter of {c.name} differs from its gradient "
                                 f"in dtype, size or place")
            _contiguous(p)

    def _momentum_of(self, ctx: Context, param):
        """The context's momentum buffer: flat f32 zeros where ``param`` lives,
        made on first use."""
        m = ctx.momentum
        if m is None or _place(m) != _place(param) or \
                hasattr(m, "data_ptr") != hasattr(param, "data_ptr"):
            if hasattr(param, "data_ptr"):
                import torch
                m = torch.zeros(param.numel(), dtype=torch.float32, device=param.device)
            else:
                import numpy as np
                m = np.zeros(param.size, dtype=np.float32)
            ctx.momentum = m
        return m

    def momentum(self, name: str):
        """The momentum buffer of a context that went through
        ``push_pull_iteration(apply=)`` (flat f32, the live buffer), or
        ``None`` before the first."""
        return self.contexts[name].momentum

    def reset_momentum(self, name: str) -> None:
        """Zero the momentum buffer; nothing to do for a context without one."""
        m = self.contexts[name].momentum
        if m is None:
            return
        if hasattr(m, "data_ptr"):
            m.zero_()
        else:
            m.fill(0)

    def _apply_iteration(self, ctxs, casts, tensors, divisor, stats, clip_norm, clip_eps, unscale,
                         apply) -> None:
        """The end of ``push_pull_iteration(apply=...)``, after the last pull:
        the compressor groups measured where ``clip_norm`` or ``stats`` asks,
        the one clip record, then the SGD step per group from the staging
        buffers.  No gradient is written."""
        names = [c.name for cs in casts.values() for c in cs]
        skipped = [c.name for c in ctxs if c.compressor is None]
        first = tensors[names[0]] if names else None
        on_dev = _place(first) is not None
        rec = None
        if clip_norm is not None or stats:
            rows = _stat_rows(len(names), first if on_dev else None)
            at = 0
            for comp, cs in casts.items():
                comp.measure_many_with([_contiguous(tensors[c.name]) for c in cs],
                                       [c.staging for c in cs], [c.extra for c in cs], divisor,
                                       plans=self._cast_plans, stats=rows[at:at + len(cs)])
                at += len(cs)
            self.grad_stats = GradStats(names, rows, skipped)
        if clip_norm is not None:
            if on_dev:
                import torch
                from .torch_ops import _red
                inv = unscale
                if inv is not None and not hasattr(inv, "data_ptr"):
                    inv = torch.tensor([float(inv)], dtype=torch.float32, device=first.device)
                with torch.cuda.device(first.device):
                    rec = _red().clip_record(rows, clip_norm, clip_eps, inv)
            else:
                from .compression import clip_record
                rec = clip_record(rows, clip_norm, clip_eps,
                                  unscale.item() if hasattr(unscale, "data_ptr") else unscale)
            self.grad_clip = GradClip(rec, names, rows, skipped)
        for comp, cs in casts.items():
            params = [apply.params[c.name] for c in cs]
            comp.apply_sgd_many(params, [c.staging for c in cs],
                                [self._momentum_of(c, p) for c, p in zip(cs, params)], divisor,
                                lr=apply.lr, momentum=apply.momentum,
                                weight_decay=apply.weight_decay, nesterov=apply.nesterov,
                                record=rec, skip_nonfinite=apply.skip_nonfinite,
                                plans=self._cast_plans)

    def _clip_iteration(self, ctxs, casts, tensors, divisor, average, clip_norm, clip_eps,
                        unscale) -> None:
        """The end of ``push_pull_iteration(clip_norm=...)``, after the last
        pull: rows of every floating context (compressor groups measured,
        uncompressed tensors by torch after their divide), one clip record,
        the scaled decompress per group and the multiply of the others."""
        comp_names = [c.name for cs in casts.values() for c in cs]
        plain = [c for c in ctxs if c.compressor is None and _is_float(tensors[c.name])]
        skipped = [c.name for c in ctxs
                   if c.compressor is None and not _is_float(tensors[c.name])]
        names = comp_names + [c.name for c in plain]
        first = tensors[names[0]] if names else None
        on_dev = hasattr(first, "data_ptr") and first.device.type == "cuda"
        rows = _stat_rows(len(names), first if on_dev else None)
        at = 0
        for comp, cs in casts.items():
            comp.measure_many_with([_contiguous(tensors[c.name]) for c in cs],
                                   [c.staging for c in cs], [c.extra for c in cs], divisor,
                                   plans=self._cast_plans, stats=rows[at:at + len(cs)])
            at += len(cs)
        for c in plain:
            if average:
                _divide_(tensors[c.name], divisor)
            _finite_row(rows[at], tensors[c.name])
            at += 1
        if on_dev:
            import torch
            from .torch_ops import _red
            inv = unscale
            if inv is not None and not hasattr(inv, "data_ptr"):
                inv = torch.tensor([float(inv)], dtype=torch.float32, device=first.device)
            with torch.cuda.device(first.device):
                rec = _red().clip_record(rows, clip_norm, clip_eps, inv)
        else:
            from .compression import clip_record
            rec = clip_record(rows, clip_norm, clip_eps,
                              unscale.item() if hasattr(unscale, "data_ptr") else unscale)
        for comp, cs in casts.items():
            comp.decompress_many_with([_contiguous(tensors[c.name]) for c in cs],
                                      [c.staging for c in cs], [c.extra for c in cs], divisor,
                                      plans=self._cast_plans, scale=rec.mult)
        for c in plain:
            _scale_(tensors[c.name], rec.mult)
        self.grad_stats = GradStats(comp_names, rows[:len(comp_names)],
                                    [c.name for c in ctxs if c.compressor is None])
        self.grad_clip = GradClip(rec, names, rows, skipped)


def _nbytes(x) -> int:
    if hasattr(x, "nbytes") and not hasattr(x, "data_ptr"):
        return int(x.nbytes)                               # numpy
    return int(x.numel() * x.element_size())               # torch


def _divide_(x, size: int) -> None:
    """In-place x /= size for a floating tensor or array."""
    if hasattr(x, "data_ptr"):                             # torch
        if not x.is_floating_point():
            raise ValueError("average needs a floating dtype")
        x.div_(size)
        return
    import numpy as np
    if not np.issubdtype(x.dtype, np.floating):
        raise ValueError("average needs a floating dtype")
    x /= size


def _contiguous(x):
    """x itself if contiguous (the casts write through it), else an error."""
    ok = x.is_contiguous() if hasattr(x, "data_ptr") else x.flags["C_CONTIGUOUS"]
    if not ok:
        raise ValueError("push_pull needs contiguous tensors")
    return x


def _zeros_like(x):
    if hasattr(x, "data_ptr"):                             # torch
        import torch
        return torch.zeros_like(x)
    import numpy as np
    return np.zeros_like(x)


def _slice(x, off: int, ln: int):
    """Byte range [off, off+ln) of a contiguous buffer, as a view of the same
    kind (pulls write through it, so a copy would lose the result)."""
    if hasattr(x, "data_ptr"):                             # torch
        import torch
        if not x.is_contiguous():
            raise ValueError("push_pull needs contiguous tensors")
        return x.reshape(-1).view(torch.uint8)[off:off + ln]
    import numpy as np
    if not x.flags["C_CONTIGUOUS"]:
        raise ValueError("push_pull needs contiguous arrays")
    return x.reshape(-1).view(np.uint8)[off:off + ln]


__all__ = ["ServerFrontend", "Worker", "Context", "GradStats", "GradClip", "SgdStep", "K_DEFAULT_PUSH_PULL", "DType", "elem_size"]
