#!/usr/bin/env python3
"""Timing of the fp16 compression casts against torch's, in one run.

At ``--elems`` elements (default 64 Mi, f32 <-> f16), over ``--sets`` rotated
buffer sets (every launch reads and writes buffers the previous one did not
touch, as bench.py's headline does), alternating the candidates round by
round so that drift hits all of them alike:

  compress        byteps_reduce_compress_fp16    vs  torch  h.copy_(x)
  decompress / 8  byteps_reduce_decompress_fp16  vs  torch  h.div_(8); out.copy_(h)
  copy            byteps_reduce_copy at the same total bytes (the project's own
                  yardstick: 0.80 of the roofline at 256 MiB)

Per candidate: the median over the rounds of (device-event time of ``--inner``
back-to-back launches) / inner, the fraction of the 8 TB/s HBM roofline that
time means for the bytes the operation must move (6 per element for both
casts; torch's two-step decompress moves 10), and the spread (max - min over
the rounds).  Gates, each against torch in the same run:

  compress    not slower than torch beyond the larger of the two spreads;
  decompress  faster than torch's two steps by more than the larger spread.

``decompress_hip_div1`` is the same pass without the divide (what the IEEE
divide costs).  Then end-to-end figures on a single GPU: a 2-worker
push_pull(average=True) round of one f32 tensor with Compression.none and
with Compression.fp16, host-resident (where the casts are the host's) and
device-resident.  One process; every GPU step runs under a
time limit of its own (a step that overruns ends the process with status
124).  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


class step:
    """A GPU step under its own time limit: past it, the process ends."""

    def __init__(self, name: str, seconds: float):
        self.name, self.seconds = name, seconds

    def _expired(self):
        print(json.dumps({"error": f"step '{self.name}' exceeded {self.seconds} s"}), flush=True)
        os._exit(124)

    def __enter__(self):
        self.timer = threading.Timer(self.seconds, self._expired)
        self.timer.daemon = True
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()
        return False


def main() -> int:
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--elems", type=int, default=64 << 20)
    p.add_argument("--sets", type=int, default=3)
    p.add_argument("--rounds", type=int, default=9)
    p.add_argument("--inner", type=int, default=24)
    p.add_argument("--warmup", type=int, default=2, help="untimed rounds")
    p.add_argument("--e2e-elems", type=int, default=16 << 20)
    p.add_argument("--e2e-iters", type=int, default=6)
    p.add_argument("--no-e2e", action="store_true")
    args = p.parse_args()

    import torch

    from prophet_amd.dtypes import DType
    from prophet_amd.reducer import GpuReducer

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    n = args.elems
    with step("setup", 120):
        red = GpuReducer(device=0)
        dev = torch.device("cuda:0")
        g = torch.Generator(device=dev).manual_seed(1)
        sets = []
        for _ in range(args.sets):
            x = torch.randn(n, device=dev, generator=g) * 64
            sets.append({"x": x, "h": torch.empty(n, dtype=torch.float16, device=dev),
                         "out": torch.empty(n, device=dev),
                         "h2": x.to(torch.float16)})
        nb = 3 * n                                   # copy: 3n bytes in + 3n out = 6 per element
        csrc = [s["x"].view(torch.uint8)[:nb] for s in sets]
        cdst = [s["out"].view(torch.uint8)[:nb] for s in sets]
        torch.cuda.synchronize()

    with step("check", 120):
        s = sets[0]
        red.compress_fp16(s["h"], s["x"], n, DType.FLOAT32)
        same_c = bool(torch.equal(s["h"].view(torch.int16), s["x"].to(torch.float16)
                                  .view(torch.int16)))
        red.decompress_fp16(s["out"], s["h"], n, DType.FLOAT32, 8)
        ref = s["h"].clone().div_(8).float()
        same_d = bool(torch.equal(s["out"].view(torch.int32), ref.view(torch.int32)))
        del ref
        torch.cuda.synchronize()

    def hip_compress(s, i):
        red.compress_fp16(s["h"], s["x"], n, DType.FLOAT32)

    def torch_compress(s, i):
        s["h"].copy_(s["x"])

    def hip_decompress(s, i):
        red.decompress_fp16(s["out"], s["h2"], n, DType.FLOAT32, 8)

    def hip_decompress_div1(s, i):     # the same pass without the divide: what the divide costs
        red.decompress_fp16(s["out"], s["h2"], n, DType.FLOAT32, 1)

    def torch_decompress(s, i):
        s["h2"].div_(8)
        s["out"].copy_(s["h2"])

    def hip_copy(s, i):
        k = i % len(sets)
        red.copy(cdst[k], csrc[k], nb)

    cands = {"compress_hip": hip_compress, "compress_torch": torch_compress,
             "decompress_hip": hip_decompress, "decompress_torch": torch_decompress,
             "decompress_hip_div1": hip_decompress_div1, "copy_hip": hip_copy}
    times = {k: [] for k in cands}
    for r in range(args.warmup + args.rounds):
        for name, fn in cands.items():
            with step(f"{name} round {r}", 60):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(args.inner):
                    fn(sets[i % len(sets)], i)
                e1.record()
                e1.synchronize()
                if r >= args.warmup:
                    times[name].append(e0.elapsed_time(e1) / args.inner)

    res = {}
    for name, ts in times.items():
        med = statistics.median(ts)
        res[name] = {"ms": round(med, 5), "min_ms": round(min(ts), 5), "max_ms": round(max(ts), 5),
                     "spread_ms": round(max(ts) - min(ts), 5),
                     "roofline_frac": round(6 * n / (med * 1e-3) / HBM_BYTES_PER_S, 4)}
    sp_c = max(res["compress_hip"]["spread_ms"], res["compress_torch"]["spread_ms"])
    sp_d = max(res["decompress_hip"]["spread_ms"], res["decompress_torch"]["spread_ms"])
    gates = {
        "compress_not_slower_than_torch":
            res["compress_hip"]["ms"] - res["compress_torch"]["ms"] <= sp_c,
        "decompress_beats_torch_two_steps":
            res["decompress_torch"]["ms"] - res["decompress_hip"]["ms"] > sp_d,
    }
    out = {"tool": "bench_compress", "elems": n, "sets": args.sets, "rounds": args.rounds,
           "inner": args.inner, "device": torch.cuda.get_device_name(0),
           "bit_equal_to_torch_device_cast": {"compress": same_c, "decompress_div8": same_d},
           "results": res, "gates": gates}
    del sets, csrc, cdst
    torch.cuda.empty_cache()

    if not args.no_e2e:
        with step("end to end", 240):
            out["push_pull_host_2workers_1gpu"] = end_to_end(args.e2e_elems, args.e2e_iters,
                                                             "host")
        with step("end to end, device tensors", 240):
            out["push_pull_device_2workers_1gpu"] = end_to_end(args.e2e_elems, args.e2e_iters,
                                                               "device")
    print(json.dumps(out), flush=True)
    return 0 if all(gates.values()) else 1


def end_to_end(nelem: int, iters: int, where: str) -> dict:
    """ms per push_pull(average=True) round of one f32 tensor (host numpy
    arrays, where the fp16 casts are the host's, or device tensors),
    2 worker threads against one PSServer on one GPU, Compression.none and
    Compression.fp16 in turn (median and spread over ``iters`` rounds after
    two untimed ones)."""
    import numpy as np
    import torch

    from prophet_amd.compression import Compression
    from prophet_amd.dtypes import DType
    from prophet_amd.pushpull import ServerFrontend, Worker
    from prophet_amd.server import PSServer

    N = 2
    res = {"elems": nelem, "workers": N, "note": f"single GPU, {where} tensors"}
    for label, comp in (("none", Compression.none), ("fp16", Compression.fp16)):
        srv = PSServer(N)
        fe = ServerFrontend(srv)
        ws = [Worker(r, fe) for r in range(N)]
        xs = [np.random.default_rng(r).standard_normal(nelem).astype(np.float32) for r in range(N)]
        if where == "device":
            xs = [torch.from_numpy(x).cuda() for x in xs]
        bar = threading.Barrier(N)
        ts, errs = [], []

        def run(w):
            try:
                w.declare("g")
                w.init_tensor("g", xs[w.rank], DType.FLOAT32, compression=comp)
                for it in range(iters + 2):
                    bar.wait(timeout=120)
                    t0 = time.perf_counter()
                    w.push_pull("g", xs[w.rank], average=True)
                    if where == "device":
                        torch.cuda.current_stream().synchronize()
                    bar.wait(timeout=120)
                    if w.rank == 0 and it >= 2:
                        ts.append((time.perf_counter() - t0) * 1e3)
            except Exception as e:
                errs.append(repr(e))
                bar.abort()
        th = [threading.Thread(target=run, args=(w,)) for w in ws]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout=200)
        srv.close()
        if errs or not ts:
            res[label] = {"error": errs}
            continue
        res[label] = {"ms": round(statistics.median(ts), 3),
                      "spread_ms": round(max(ts) - min(ts), 3)}
    if "ms" in res.get("none", {}) and "ms" in res.get("fp16", {}):
        res["fp16_over_none"] = round(res["fp16"]["ms"] / res["none"]["ms"], 3)
    return res


if __name__ == "__main__":
    sys.exit(main())
