"""Device operands of one fold between guard bytes, for the GPU parity tests.
A helper module, not a conftest.

Operands puts every source and dst `offset` bytes past a 256-byte boundary of
a buffer of its own, filled with 0xEE; dst is prefilled with 0x5A (or is
srcs[0], in place).  result() returns dst's bytes after checking that the
guard bytes on both sides of dst and of every source are still 0xEE and that
no source changed (but srcs[0] when it is dst).

The operand map says which operands are one buffer: `alias` is the index of
the source that dst is (None: a buffer of its own; `inplace=True` is alias 0),
and `same` lists groups of source indices that share one buffer (duplicate
sources; a group's offsets are its first member's, and load() takes the same
bytes for every member).  The guarantees hold per distinct buffer: guard bytes
around each, and every buffer that is not dst's unchanged."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

GUARD, FILL = 0xEE, 0x5A
PAD = 256           # guard bytes before and after every operand


class Operands:
    def __init__(self, dev, n_src: int, L: int, src_offs=None, dst_off: int = 16,
                 inplace: bool = False, alias=None, same=()):
        if inplace:
            assert alias in (None, 0)
            alias = 0
        self.L, self.alias, self.inplace = L, alias, alias is not None
        self.src_offs = list(src_offs) if src_offs is not None else [0] * n_src
        assert len(self.src_offs) == n_src
        # first[k]: the source whose buffer source k is
        self.first = list(range(n_src))
        for group in same:
            for k in group:
                assert self.first[k] == k and k >= group[0]
                self.first[k] = group[0]
                self.src_offs[k] = self.src_offs[group[0]]
        self.src_bufs = []
        for k, o in enumerate(self.src_offs):
            self.src_bufs.append(self._buffer(dev, o) if self.first[k] == k
                                 else self.src_bufs[self.first[k]])
        assert alias is None or 0 <= alias < n_src
        self.dst_off = dst_off if alias is None else self.src_offs[alias]
        self.dst_buf = self._buffer(dev, dst_off) if alias is None else self.src_bufs[alias]
        self.held = None            # host bytes of the sources, as loaded
        for b in self.src_bufs + [self.dst_buf]:
            assert b.data_ptr() % 256 == 0

    def _buffer(self, dev, off):
        return torch.full((PAD + off + self.L + PAD,), GUARD, dtype=torch.uint8, device=dev)

    @staticmethod
    def _view(buf, off, L):
        return buf[PAD + off:PAD + off + L]

    @property
    def src_views(self):
        return [self._view(b, o, self.L) for b, o in zip(self.src_bufs, self.src_offs)]

    @property
    def dst_view(self):
        return self._view(self.dst_buf, self.dst_off, self.L)

    @property
    def srcs(self):
        return [b.data_ptr() + PAD + o for b, o in zip(self.src_bufs, self.src_offs)]

    @property
    def dst(self):
        return self.dst_buf.data_ptr() + PAD + self.dst_off

    @property
    def bucket(self):
        return (self.dst, self.srcs, self.L)

    def load(self, ins):
        """Sources from host byte arrays (or pinned host tensors); a separate
        dst back to 0x5A."""
        assert len(ins) == len(self.src_bufs)
        self.held = ins
        if not self.L:
            return self
        for k, (v, x) in enumerate(zip(self.src_views, ins)):
            assert len(x) == self.L
            if self.first[k] != k:          # a duplicate: its group's one input
                assert x is ins[self.first[k]], f"sources {self.first[k]} and {k} share a buffer"
                continue
            v.copy_(x if isinstance(x, torch.Tensor) else torch.from_numpy(x), non_blocking=True)
        if not self.inplace:
            self.dst_view.fill_(FILL)
        return self

    def result(self) -> np.ndarray:
        whole = self.dst_buf.cpu().numpy()
        lo = PAD + self.dst_off
        assert bool((whole[:lo] == GUARD).all()), "bytes before dst changed"
        assert bool((whole[lo + self.L:] == GUARD).all()), "bytes after dst changed"
        for k, (b, o, x) in enumerate(zip(self.src_bufs, self.src_offs, self.held)):
            if b is self.dst_buf or self.first[k] != k:     # dst's buffer; checked with its first
                continue
            h = b.cpu().numpy()
            x = x.numpy() if isinstance(x, torch.Tensor) else x
            assert np.array_equal(h[PAD + o:PAD + o + self.L], x), f"source {k} changed"
            assert bool((h[:PAD + o] == GUARD).all()), f"bytes before source {k} changed"
            assert bool((h[PAD + o + self.L:] == GUARD).all()), f"bytes after source {k} changed"
        return whole[lo:lo + self.L]


    def untouched(self, what=""):
        """After a refused call: every buffer, dst's included, holds what
        load() left — guard bytes, the sources' bytes, 0x5A in a dst of its own."""
        bufs = [(b, o, x) for k, (b, o, x) in
                enumerate(zip(self.src_bufs, self.src_offs, self.held)) if self.first[k] == k]
        if self.alias is None:
            bufs.append((self.dst_buf, self.dst_off, np.full(self.L, FILL, np.uint8)))
        for i, (b, o, x) in enumerate(bufs):
            h = b.cpu().numpy()
            x = x.numpy() if isinstance(x, torch.Tensor) else x
            assert np.array_equal(h[PAD + o:PAD + o + self.L], x), f"{what}: buffer {i} changed"
            assert bool((h[:PAD + o] == GUARD).all()) and bool((h[PAD + o + self.L:] == GUARD).all()), \
                f"{what}: guard bytes of buffer {i} changed"


class Guarded:
    """One device buffer of L bytes `off` bytes past a 256-byte boundary
    between 0xEE guard bytes (a rank's whole vector or a receive slot of the
    shard tests): `ptr`, load(host bytes), and bytes() -> its L bytes after
    checking the guard bytes."""

    def __init__(self, dev, L: int, off: int = 0):
        self.L, self.off = L, off
        self.buf = torch.full((PAD + off + L + PAD,), GUARD, dtype=torch.uint8, device=dev)
        assert self.buf.data_ptr() % 256 == 0

    @property
    def ptr(self):
        return self.buf.data_ptr() + PAD + self.off

    def load(self, x):
        self.buf[PAD + self.off:PAD + self.off + self.L].copy_(torch.from_numpy(x))
        return self

    def bytes(self, what="") -> np.ndarray:
        h = self.buf.cpu().numpy()
        lo = PAD + self.off
        assert bool((h[:lo] == GUARD).all()) and bool((h[lo + self.L:] == GUARD).all()), \
            f"{what}: guard bytes changed"
        return h[lo:lo + self.L]


def run_sum_n(red, dev, dt, ins, L, src_offs=None, dst_off=16, inplace=False, mode=0,
              alias=None, same=()):
    """byteps_reduce_sum_n of host byte arrays `ins` at byte offsets `src_offs`
    into dst at `dst_off` (or into srcs[0]); Operands' checks; dst's L bytes."""
    ops = Operands(dev, len(ins), L, src_offs, dst_off, inplace, alias, same).load(ins)
    torch.cuda.synchronize()
    red.sum_n(ops.dst, ops.srcs, L, dt, mode=mode)
    torch.cuda.synchronize()
    return ops.result()


def assert_elements(dt, got, want, kind, what):
    """Raw bytes; a mismatch names the first elements and their probe kinds.
    Trailing bytes behind the last whole element are compared as bytes."""
    from prophet_amd.dtypes import elem_size
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if np.array_equal(got, want):
        return
    es = elem_size(dt)
    U = np.dtype(f"u{es}")
    n = len(want) // es
    g, w = got[:n * es].view(U), want[:n * es].view(U)
    bad = np.flatnonzero(g != w)
    k = (lambda i: int(kind[i])) if kind is not None else (lambda i: -1)
    raise AssertionError(
        f"{what}: {len(bad)} of {n} elements differ"
        f"{'' if np.array_equal(got[n * es:], want[n * es:]) else ', trailing bytes too'}; first "
        + ", ".join(f"[{i}] kind {k(i)} got {int(g[i]):#x} want {int(w[i]):#x}" for i in bad[:6]))
