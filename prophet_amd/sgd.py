"""The SGD step inside the decompress: the host definition.

``apply_sgd`` (``byteps_reduce_cast_plan_apply_sgd``,
``prophet_amd/csrc/bpsr_cast_sgd.h``) takes the pulled 2-byte aggregate
straight into the parameters: one pass reads the wire, the float32 parameter
``p`` and the float32 momentum buffer ``m`` and writes the last two in place;
the gradient is never written.  The HIP kernels are pinned bit for bit to the
numpy lines below; host tensors and numpy arrays go through them.

Per element, every line ONE IEEE float32 operation, rounded to nearest even,
subnormals kept, nothing fused; ``lr``, ``mu``, ``wd`` and ``mult`` are
float32 values::

    h  = the wire value; for divisor > 1: wire(f32(h) / divisor)
    g  = f32(h)                                  # exact
    g  = g * mult          only with a clip record (the scaled decompress)
    g  = g + wd * p        only when wd != 0
    m' = mu * m + g
    d  = g + mu * m'       if nesterov else m'
    p' = p - lr * d

The momentum buffer always exists and starts as zeros: the first step is then
torch's ``buf = grad``, as values.  ``mu == 0`` follows the formula literally.
NaN payloads are not pinned, NaN-ness is.  Wherever every product and sum is
exact this is ``torch.optim.SGD(foreach=False)``; on general inputs torch's
vectorised ``add_(alpha=)`` may fuse a multiply into an add, which this never
does.
"""
from __future__ import annotations

import numpy as np

WIRES = ("fp16", "bf16")


def check_hyper(lr, momentum=0.0, weight_decay=0.0, nesterov=False) -> None:
    """The hyper-parameter rules of ``byteps_reduce_cast_plan_apply_sgd``, on
    the float32 values the step uses."""
    lr, mu, wd = np.float32(lr), np.float32(momentum), np.float32(weight_decay)
    if not np.isfinite(lr):
        raise ValueError(f"lr {lr} is not finite")
    if not (mu >= 0 and mu < 1):
        raise ValueError(f"momentum {mu} is not in [0, 1)")
    if not (wd >= 0 and np.isfinite(wd)):
        raise ValueError(f"weight_decay {wd} is not a finite number >= 0")
    if nesterov and mu == 0:
        raise ValueError("nesterov needs a momentum above 0")


def _bf16_rne(x):
    """float32 array to bf16 bits, round to nearest even; a NaN stays a NaN."""
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)
    nan = np.isnan(x)
    return np.where(nan, ((u >> np.uint64(16)) | np.uint64(0x40)).astype(np.uint16), r)


def wire_to_f32(h, wire: str, divisor: int = 1):
    """The gradient a wire buffer carries: ``h`` (uint16 bits, or float16 for
    the fp16 wire) widened exactly, after ``wire(f32(h) / divisor)`` for a
    divisor above 1 — the decompress's divide, on the 2-byte value."""
    if wire not in WIRES:
        raise ValueError(f"wire {wire!r}: one of {WIRES}")
    if int(divisor) < 1:
        raise ValueError(f"divisor {divisor} < 1")
    bits = np.ascontiguousarray(h).reshape(-1).view(np.uint16)
    if wire == "fp16":
        g = bits.view(np.float16).astype(np.float32)
    else:
        g = (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)
    if int(divisor) > 1:
        with np.errstate(all="ignore"):
            q = g / np.float32(int(divisor))
            if wire == "fp16":
                g = q.astype(np.float16).astype(np.float32)
            else:
                g = (_bf16_rne(q).astype(np.uint32) << np.uint32(16)).view(np.float32)
    return g


def sgd_step(p, m, h, wire: str, divisor: int = 1, *, lr, momentum=0.0, weight_decay=0.0,
             nesterov=False, mult=None):
    """One step: ``(p', m')`` as new float32 arrays from the float32 arrays
    ``p`` and ``m`` and the wire buffer ``h``.  ``mult``: a clip record's
    multiplier, or None for no record."""
    g = wire_to_f32(h, wire, divisor)
    if mult is not None:
        with np.errstate(all="ignore"):
            g = g * np.float32(mult)
    return sgd_update(p, m, g, lr=lr, momentum=momentum, weight_decay=weight_decay,
                      nesterov=nesterov)


def sgd_update(p, m, g, *, lr, momentum=0.0, weight_decay=0.0, nesterov=False):
    """The step from the float32 gradient ``g`` on (widened, divided and
    multiplied already): ``(p', m')``."""
    check_hyper(lr, momentum, weight_decay, nesterov)
    lr, mu, wd = np.float32(lr), np.float32(momentum), np.float32(weight_decay)
    p = np.ascontiguousarray(p, dtype=np.float32).reshape(-1)
    m = np.ascontiguousarray(m, dtype=np.float32).reshape(-1)
    g = np.ascontiguousarray(g, dtype=np.float32).reshape(-1)
    if not p.size == m.size == g.size:
        raise ValueError(f"sgd step: {p.size} parameters, {m.size} momenta, {g.size} gradients")
    with np.errstate(all="ignore"):
        if wd != 0:
            t = wd * p
            g = g + t
        t = mu * m
        mn = t + g
        if nesterov:
            t = mu * mn
            d = g + t
        else:
            d = mn
        t = lr * d
        pn = p - t
    return pn, mn


__all__ = ["WIRES", "check_hyper", "wire_to_f32", "sgd_step", "sgd_update"]
