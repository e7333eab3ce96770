"""The server round of a packed wire (``Compression.onebit_ef``, DESIGN.md
§11.11; ``Compression.mxfp8_ef`` / ``mxfp4_ef``, §11.17;
``Compression.topk_ef.at(ratio)``, §11.18): request type
``kCompressedPushPull``.

The element-wise server cannot fold a packed payload.  ``PackedRound`` is the
store ``ServerFrontend`` hands such requests to: per key it keeps the key's
compressor, one payload slot a worker, an f32 residual of its own, the output
payload and a round counter.  The last arrival of a round runs the compressor's
``refold_many_into`` — decode the N payloads, sum, compress the sum against the
store's residual — and every worker pulls 1, 8.25 or 4.25 bits an element back.

A key's wire is read from its init payload's header.  The fourth word first:
``topk.INIT_TAG`` there is a top-k key (``{k, n_lo, n_hi, tag}``; ``k`` may be
0, 4 or 8 like any other number, so the first word cannot name this wire), its
compressor the ``TopKEFCompressor.at(ratio)`` among the store's wires whose
payload of ``n`` elements has those ``16 + 8 k`` bytes.  Every other wire leaves
that word zero and is named by the first: 0 is the 1-bit wire (``{0.0f, n}``),
8 or 4 a block-scaled one (``{bits, n_lo, n_hi, 0}``).  Init payloads are never
folded, so the tag reaches no kernel.

Keys live where their first pushed payload lives: a device (a cached refold
plan on the store's own stream: three launches for the 1-bit wire, one for a
block-scaled one, the compress's ten for top-k) or numpy on the host
(``onebit.refold``, ``mx.refold``, ``topk.refold``).
Device work is ordered by events, never by a device-wide sync:

* a push copies into the worker's slot on the pusher's current stream, after
  the refold that last read the slot, and records the slot's event;
* the refold waits for every slot's event and for every pull copy of the round
  before (a worker pulls round t before it pushes round t + 1, so those events
  all exist when round t + 1 completes), and records the round's event;
* a pull makes the caller's current stream wait for the round's event, copies
  the output payload out and records an event of its own.

The init push establishes a key and is the workers' barrier: it carries the
payload of ``n`` zeros (header ``{0.0, n}``) built on the host, returns once
every worker's init push arrived, runs no refold and leaves the residual zero.
"""
from __future__ import annotations

import threading

import numpy as np

from . import onebit, topk
from .compression import (CastPlanCache, MXFP4EFCompressor, MXFP8EFCompressor,
                          OneBitEFCompressor, TopKEFCompressor)

# the first word of an init payload's header: the key's compressor
_WIRES = {0: OneBitEFCompressor, 8: MXFP8EFCompressor, 4: MXFP4EFCompressor}


def _is_device(x) -> bool:
    return hasattr(x, "data_ptr") and x.device.type == "cuda"


def _host_bytes(x):
    """A host payload (numpy array or CPU tensor) as a flat uint8 array."""
    a = x.detach().numpy() if hasattr(x, "data_ptr") else np.asarray(x)
    return a.reshape(-1).view(np.uint8)


class _Key:
    """One key's state; everything under ``cond``."""

    def __init__(self, comp, n: int, nbytes: int):
        self.comp, self.n, self.nbytes = comp, n, nbytes
        self.cond = threading.Condition()
        self.inited: set = set()          # workers whose init push arrived
        self.arrived: set = set()         # workers that pushed the open round
        self.pushed: dict = {}            # worker -> rounds pushed so far
        self.round = 0                    # rounds complete
        self.device = None                # set by the first payload: a device or "host"
        self.slots = self.resid = self.out = None
        self.plans = None                 # device: the key's refold plan
        self.slot_events: dict = {}       # device: worker -> its slot copy
        self.pull_events: list = []       # device: the pull copies of the last round
        self.round_event = None           # device: the last refold


class PackedRound:
    """The packed-payload store of ``num_workers`` workers; ``wires``: the
    compressors whose keys it takes (the 1-bit wire unless named)."""

    def __init__(self, num_workers: int, wires=(OneBitEFCompressor,)):
        if int(num_workers) < 1 or int(num_workers) > onebit.MAX_SRCS:
            raise ValueError(f"a packed round takes 1..{onebit.MAX_SRCS} workers, "
                             f"got {num_workers}")
        self.num_workers = int(num_workers)
        self.wires = tuple(wires)
        self._keys: dict = {}
        self._lock = threading.Lock()
        self._streams: dict = {}          # device -> the store's own stream

    def owns(self, key: int) -> bool:
        return key in self._keys

    def residual(self, key: int):
        """The store's f32 residual of ``key`` (the live buffer), or None
        before the first round."""
        return self._keys[key].resid

    # ---------------------------------------------------------------- push
    def push(self, key: int, worker: int, data, nbytes: int) -> None:
        if not 0 <= int(worker) < self.num_workers:
            raise ValueError(f"worker {worker} outside 0..{self.num_workers - 1}")
        with self._lock:
            k = self._keys.get(key)
            if k is None:
                # the first init push: sizes come from the header it carries
                if _is_device(data):
                    raise ValueError(f"key {key}: the init push is built on the host")
                head = _host_bytes(data)[:onebit.HEADER_BYTES]
                word, n = int(head[0:4].view("<u4")[0]), int(head[4:12].view("<u8")[0])
                if int(head[12:16].view("<u4")[0]) == topk.INIT_TAG:
                    # a top-k key: the first word is its k, any of 1..n
                    if not 1 <= word <= n or int(nbytes) != topk.payload_bytes(word):
                        raise ValueError(f"key {key}: a top-k init payload of {nbytes} bytes for "
                                         f"k {word} of {n} elements")
                    tk = [w for w in self.wires
                          if isinstance(w, type) and issubclass(w, TopKEFCompressor)]
                    comp = next((w for w in tk if w.RATIO is not None
                                 and w.payload_nbytes(n) == int(nbytes)), None)
                else:
                    comp = _WIRES.get(word)
                if comp is None or comp not in self.wires:
                    raise ValueError(f"key {key}: an init payload of a wire this store does not "
                                     f"refold (header word {word:#x})")
                if comp.payload_nbytes(n) != int(nbytes):
                    raise ValueError(f"key {key}: an init payload of {nbytes} bytes for {n} "
                                     f"elements")
                k = self._keys[key] = _Key(comp, n, int(nbytes))
        if int(nbytes) != k.nbytes or _nbytes(data) != k.nbytes:
            raise ValueError(f"key {key}: a payload of {nbytes} bytes, the key's has {k.nbytes}")
        with k.cond:
            if worker not in k.inited:
                k.inited.add(worker)
                k.cond.notify_all()
                k.cond.wait_for(lambda: len(k.inited) == self.num_workers)
                return
            if worker in k.arrived:
                raise ValueError(f"key {key}: worker {worker} pushed twice in one round")
            if k.device is None:
                self._place(k, data)
            if (k.device == "host") == _is_device(data):
                raise ValueError(f"key {key}: its payloads live on {k.device}")
            if k.device == "host":
                np.copyto(k.slots[worker], _host_bytes(data))
            else:
                self._copy_in(k, worker, data)
            k.arrived.add(worker)
            k.pushed[worker] = k.pushed.get(worker, 0) + 1
            if len(k.arrived) == self.num_workers:
                self._refold(k)
                k.arrived.clear()
                k.round += 1
                k.cond.notify_all()

    def _place(self, k: _Key, data) -> None:
        """The key's buffers, where its first payload lives; the residual zero."""
        if not _is_device(data):
            k.device = "host"
            k.slots = [np.zeros(k.nbytes, np.uint8) for _ in range(self.num_workers)]
            k.resid = np.zeros(k.n, np.float32)
            k.out = np.zeros(k.nbytes, np.uint8)
            return
        import torch
        k.device = data.device
        k.slots = [torch.zeros(k.nbytes, dtype=torch.uint8, device=k.device)
                   for _ in range(self.num_workers)]
        k.resid = torch.zeros(k.n, dtype=torch.float32, device=k.device)
        k.out = torch.zeros(k.nbytes, dtype=torch.uint8, device=k.device)
        k.plans = CastPlanCache(1)
        # the zeroing above ran on this thread's stream: the first refold and
        # the other workers' first slot copies come after it
        k.round_event = torch.cuda.Event()
        k.round_event.record(torch.cuda.current_stream(k.device))

    def _stream(self, device):
        import torch
        with self._lock:
            s = self._streams.get(device)
            if s is None:
                s = self._streams[device] = torch.cuda.Stream(device)
            return s

    def _copy_in(self, k: _Key, worker: int, data) -> None:
        import torch
        cur = torch.cuda.current_stream(k.device)
        cur.wait_event(k.round_event)     # the refold that last read the slot
        k.slots[worker].copy_(data.reshape(-1), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(cur)
        k.slot_events[worker] = ev

    def _refold(self, k: _Key) -> None:
        """The round of one key, by its last arrival."""
        if k.device == "host":
            k.comp.refold_many_into([k.out], [k.resid], [k.slots])
            return
        import torch
        st = self._stream(k.device)
        for ev in list(k.slot_events.values()) + k.pull_events:
            st.wait_event(ev)
        k.pull_events = []
        with torch.cuda.stream(st):
            k.comp.refold_many_into([k.out], [k.resid], [k.slots], plans=k.plans)
        k.round_event = torch.cuda.Event()
        k.round_event.record(st)

    # ---------------------------------------------------------------- pull
    def pull(self, key: int, worker: int, out, nbytes: int) -> None:
        """The output payload of the last round ``worker`` pushed, once that
        round is complete."""
        k = self._keys[key]
        if int(nbytes) != k.nbytes or _nbytes(out) != k.nbytes:
            raise ValueError(f"key {key}: a pull of {nbytes} bytes, the key's payload has "
                             f"{k.nbytes}")
        with k.cond:
            want = k.pushed.get(worker, 0)
            if want == 0:
                raise ValueError(f"key {key}: worker {worker} pushed nothing")
            k.cond.wait_for(lambda: k.round >= want)
            if k.device == "host":
                if _is_device(out):
                    raise ValueError(f"key {key}: its payloads live on the host")
                np.copyto(_host_bytes(out), k.out)
                return
            import torch
            cur = torch.cuda.current_stream(k.device)
            cur.wait_event(k.round_event)
            out.reshape(-1).copy_(k.out, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cur)
            k.pull_events.append(ev)

    def close(self) -> None:
        for k in self._keys.values():
            if k.plans is not None:
                k.plans.close()
        self._keys.clear()


def _nbytes(x) -> int:
    if hasattr(x, "data_ptr"):
        return int(x.numel() * x.element_size())
    return int(np.asarray(x).nbytes)


__all__ = ["PackedRound"]
