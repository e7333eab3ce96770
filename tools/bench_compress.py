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

``--iteration`` measures what a whole iteration's casts cost instead: the 165
entries of tools/cfg3_resnet50_table.txt (ResNet-50's gradients as fp16 byte
ranges), each one f32 segment of len / 2 elements at its own offset in one
arena per side, compressed and then decompressed (divisor 8) by

  loop    one compress_fp16_out and one decompress_fp16_out per segment — what
          push_pull_iteration queued before cast plans: 2 x 165 launches;
  plan    one cast-plan launch each way (byteps_reduce_cast_plan_*);
  single  for scale, one one-tensor call each way over the same element count.

Same method: rotated buffer sets, candidates alternated round by round,
medians of rounds, device events.  Then one 64 Mi-element segment, each
direction on its own, as a plan launch and as the one-tensor call.  Gates:

  iteration  plan faster than loop by more than the larger of the two spreads;
  big        per direction, the plan's median within the larger of the two
             spreads of the one-tensor call's.

One JSON line, also appended to ``--out`` when given.

``--wire bf16`` measures the bf16 wire (byteps_reduce_compress_to /
_decompress_from / _cast_plan_create_wire with BFLOAT16) against the fp16 wire
in the same run, by the same method, the two alternated round by round: at
``--elems`` the one-tensor compress and decompress / 8 of f32, with
``--iteration`` the plan over the ResNet-50 table, each direction timed on its
own.  Both wires move the same 6 bytes per f32 element.  Gates, per direction:

  the bf16 median is not slower than the fp16 median by more than the larger
  of the two candidates' spreads (max - min of the rounds).

``--wire fp16`` (the default) is everything above, unchanged.

``--ef`` measures the error-feedback compress (byteps_reduce_compress_ef, wire
``--wire``) in one run, by the same method, the candidates alternated round by
round, at ``--elems`` f32 elements:

  ef_hip     the fused pass: reads g and r, writes the wire and r' (14 B an
             element);
  ef_torch   torch's four-step composition on the same buffers — add, cast, cast
             back, sub (at least 36 B an element; it leaves out the isfinite
             select, which would only add to it);
  plain_hip  the plain compress (6 B an element), for scale.

and over the ResNet-50 table (165 segments, each with its own residual) one EF
plan launch against 165 one-tensor launches.  Roofline fractions are on the
bytes each candidate must move (14, 36 and 6 an element).  Gates:

  ef_hip faster than ef_torch by more than the larger of the two spreads;
  the EF plan faster than the loop by more than the larger of the two spreads.

``--sr`` measures the stochastic-rounding compress (byteps_reduce_compress_sr)
in one run, by the same method, the candidates alternated round by round, at
``--elems`` f32 elements:

  sr_bf16, sr_fp16  the fused pass on either wire (6 B an element);
  sr_bf16_head7     the same with the wide base one element past a 16-byte
                    boundary: the cut's head is 7, every 16-byte vector
                    straddles two Philox groups and draws both;
  plain_hip         the plain compress of ``--wire`` (6 B an element);
  ef_hip            the fused error-feedback compress of ``--wire`` (14 B);
  sr_torch          torch's own composition for bf16 on the same buffers:
                    randint, integer add on the viewed bits, shift, narrow (at
                    least 26 B an element).

and over the ResNet-50 table (165 segments, each under its own key) one SR plan
launch against 165 one-tensor launches.  The first 1 Mi elements of each wire
are compared with the numpy definition (prophet_amd/sr.py).  Gates:

  sr_bf16 faster than sr_torch by more than the SUM of the two spreads;
  the SR plan faster than the loop by more than the larger of the two spreads.

``--stats`` measures the decompress with statistics
(byteps_reduce_cast_plan_decompress_stats: per segment the sum of squares and
the non-finite count of what the decompress writes) in one
run, by the same method, the candidates alternated round by round, over the
ResNet-50 table (165 f32 segments, divisor 8) and over one ``--elems`` segment:

  plan        the plain plan decompress (6 B an element);
  plan_stats  the decompress with statistics, both kernels (6 B an element);
  torch       the plain plan decompress followed by what a user writes today —
              table: torch._foreach_norm over the 165 outputs, stack, norm, and
              isfinite over the stacked norms (GradScaler's way: a non-finite
              element makes its tensor's norm non-finite); one segment:
              vector_norm and isfinite of it.  A second read of every output:
              10 B an element at least.

The statistics are compared with torch's f64 arithmetic on the device first
(counts exact, sums within nelem * 2^-52).  Gate, at both shapes:

  plan_stats faster than torch by more than the larger of the two spreads.

``plan_stats / plan`` is recorded, not gated.

``--clip`` measures clipping by the global norm and unscaling inside the
decompress by the same method over the same two shapes
(fp16 wire unless ``--wire bf16``, f32, divisor 8, unscale 2^-7, a max_norm
that clips):

  clip_fused        byteps_reduce_cast_plan_measure, byteps_reduce_clip_record,
                    byteps_reduce_cast_plan_decompress_scaled: 2 B read, then
                    2 B read + 4 B written an element;
  stats_then_torch  the decompress with statistics, the record's arithmetic
                    from the rows in torch, torch._foreach_mul_ over the
                    outputs: 6 + 8 B an element;
  torch_all         the plain plan decompress, then
                    torch.nn.utils.clip_grad_norm_(foreach=True) on the
                    outputs: 6 + 4 + 8 B an element (it does not unscale).

The fused outputs are first compared bit for bit with ``mult`` times the plain
decompress and the measured rows with the statistics rows.  Gate, at both
shapes:

  clip_fused faster than the faster of the other two by more than the larger
  of the two spreads.

``--sgd`` measures the SGD step inside the decompress by the
same method over the same two shapes (f32, divisor 8, unscale 2^-7, a max_norm
that clips, lr 1e-3, momentum 0.9, weight decay 1e-4, nesterov).  Every
candidate ends with updated parameters and momenta, each on its own:

  apply           measure, clip record, byteps_reduce_cast_plan_apply_sgd with
                  the record and skip_nonfinite: 2 + 18 B an element;
  scaled_fused    measure, clip record, the scaled decompress into the
                  gradients, torch.optim.SGD(fused=True).step(): 2 + 6 + 20 B;
  scaled_foreach  the same with foreach=True;
  apply_only, scaled_fused_only   the last launch of ``apply`` (18 B) and the
                  last two of ``scaled_fused`` (26 B) alone, the record given.

The parameters and momenta after ``apply`` are first compared bit for bit with
the definition evaluated by torch one op at a time on the scaled decompress's
output.  Gate, at both shapes:

  apply faster than the faster of scaled_fused and scaled_foreach by more than
  the larger of the two spreads.
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
    p.add_argument("--iteration", action="store_true",
                   help="a whole iteration's casts: per-segment loop, cast plan, one tensor")
    p.add_argument("--table", default=os.path.join(ROOT, "tools", "cfg3_resnet50_table.txt"))
    p.add_argument("--out", default=None, help="append the JSON line to this file too")
    p.add_argument("--wire", choices=("fp16", "bf16"), default="fp16",
                   help="bf16: the bf16 casts alternated with the fp16 casts")
    p.add_argument("--ef", action="store_true",
                   help="the error-feedback compress against torch's composition and the "
                        "plain compress; the ResNet-50 table as one EF plan")
    p.add_argument("--sr", action="store_true",
                   help="the stochastic-rounding compress against torch's composition, the "
                        "plain and the error-feedback compress; the ResNet-50 table as one SR plan")
    p.add_argument("--stats", action="store_true",
                   help="the decompress with statistics against the plain decompress and "
                        "torch's norm + isfinite after it; the ResNet-50 table and one segment")
    p.add_argument("--clip", action="store_true",
                   help="clip by global norm and unscale inside the decompress against the "
                        "statistics decompress + torch's multiply and against "
                        "clip_grad_norm_; the ResNet-50 table and one segment")
    p.add_argument("--sgd", action="store_true",
                   help="the SGD step inside the decompress against the scaled decompress "
                        "followed by torch's fused and foreach SGD; the ResNet-50 table and "
                        "one segment")
    args = p.parse_args()
    if args.sgd:
        return sgd_mode(args)
    if args.clip:
        return clip_mode(args)
    if args.stats:
        return stats_mode(args)
    if args.sr:
        return sr_mode(args)
    if args.ef:
        return ef_mode(args)
    if args.wire == "bf16":
        return wire_mode(args)
    if args.iteration:
        return iteration_mode(args)

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


def read_table(path: str):
    """(offset, len) in fp16 bytes of every entry of a cfg3 table file."""
    with open(path) as f:
        total, count, _ = (int(v) for v in f.readline().split())
        rows = [tuple(int(v) for v in line.split()) for line in f if line.strip()]
    rows = rows[:count]
    if len(rows) != count or max(o + ln for o, ln in rows) > total:
        raise ValueError(f"{path}: {len(rows)} entries, header says {count} in {total} bytes")
    return total, rows


def timed_rounds(torch, cands, nsets, args):
    """Per candidate the per-call device-event times of every timed round:
    ``cands[name] = (fn(set index), calls per round)``."""
    times = {k: [] for k in cands}
    for r in range(args.warmup + args.rounds):
        for name, (fn, inner) in cands.items():
            with step(f"{name} round {r}", 60):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(inner):
                    fn(i % nsets)
                e1.record()
                e1.synchronize()
                if r >= args.warmup:
                    times[name].append(e0.elapsed_time(e1) / inner)
    return {name: {"ms": round(statistics.median(ts), 5), "min_ms": round(min(ts), 5),
                   "max_ms": round(max(ts), 5), "spread_ms": round(max(ts) - min(ts), 5),
                   "calls_per_round": cands[name][1]}
            for name, ts in times.items()}


def iteration_mode(args) -> int:
    import torch

    from prophet_amd import torch_ops  # noqa: F401  (registers torch.ops.bpsr.*)
    from prophet_amd.dtypes import DType
    from prophet_amd.reducer import GpuReducer

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    total_bytes, rows = read_table(args.table)
    dev = torch.device("cuda:0")
    comp, decomp = torch.ops.bpsr.compress_fp16_out, torch.ops.bpsr.decompress_fp16_out
    with step("setup", 120):
        red = GpuReducer(device=0)
        g = torch.Generator(device=dev).manual_seed(2)
        nelem = sum(ln // 2 for _, ln in rows)
        sets = []
        for _ in range(args.sets):
            wide = torch.randn(total_bytes // 2, device=dev, generator=g) * 64
            half = torch.empty(total_bytes // 2, dtype=torch.float16, device=dev)
            segs = [(wide[o // 2:(o + ln) // 2], half[o // 2:(o + ln) // 2]) for o, ln in rows]
            sets.append({"wide": wide, "half": half, "segs": segs,
                         "plan": red.cast_plan([(w, h, w.numel()) for w, h in segs],
                                               DType.FLOAT32),
                         "one_w": wide[:nelem], "one_h": half[:nelem]})
        torch.cuda.synchronize()

    with step("check", 120):
        s = sets[0]
        s["plan"].compress()
        ref = torch.full_like(s["half"], 7.0)
        for w, h in s["segs"]:
            o = h.data_ptr() - s["half"].data_ptr()
            comp(ref[o // 2:o // 2 + h.numel()], w)
        same_c = all(bool(torch.equal(h.view(torch.int16),
                                      ref[(h.data_ptr() - s["half"].data_ptr()) // 2:][:h.numel()]
                                      .view(torch.int16))) for _, h in s["segs"])
        s["plan"].decompress(8)
        same_d = True
        for w, h in s["segs"]:
            one = torch.empty_like(w)
            decomp(one, h, 8)
            same_d = same_d and bool(torch.equal(w.view(torch.int32), one.view(torch.int32)))
        del ref
        torch.cuda.synchronize()

    def loop(k):
        for w, h in sets[k]["segs"]:
            comp(h, w)
        for w, h in sets[k]["segs"]:
            decomp(w, h, 8)

    def plan(k):
        sets[k]["plan"].compress()
        sets[k]["plan"].decompress(8)

    def single(k):
        red.compress_fp16(sets[k]["one_h"], sets[k]["one_w"], nelem, DType.FLOAT32)
        red.decompress_fp16(sets[k]["one_w"], sets[k]["one_h"], nelem, DType.FLOAT32, 8)

    few = max(1, args.inner // 8)            # 330 launches a call: fewer calls a round
    res = timed_rounds(torch, {"loop": (loop, few), "plan": (plan, args.inner),
                               "single": (single, args.inner)}, len(sets), args)
    sp = max(res["loop"]["spread_ms"], res["plan"]["spread_ms"])
    gates = {"iteration_plan_beats_loop": res["loop"]["ms"] - res["plan"]["ms"] > sp}
    out = {"tool": "bench_compress", "mode": "iteration", "table": os.path.basename(args.table),
           "segments": len(rows), "elems": nelem, "bytes_moved_per_iteration": 12 * nelem,
           "sets": args.sets, "rounds": args.rounds, "inner": args.inner,
           "device": torch.cuda.get_device_name(0),
           "bit_equal_to_per_segment_calls": {"compress": same_c, "decompress_div8": same_d},
           "iteration": res, "iteration_gate_spread_ms": sp,
           "loop_over_plan": round(res["loop"]["ms"] / res["plan"]["ms"], 2),
           "plan_over_single": round(res["plan"]["ms"] / res["single"]["ms"], 3)}
    for s in sets:
        s["plan"].close()
    del sets
    torch.cuda.empty_cache()

    n = args.elems
    with step("setup, one segment", 120):
        big = []
        for _ in range(args.sets):
            x = torch.randn(n, device=dev, generator=g) * 64
            h = x.to(torch.float16)
            big.append({"x": x, "h": h, "h_out": torch.empty_like(h),
                        "pc": red.cast_plan([(x, torch.empty_like(h), n)], DType.FLOAT32)})
        for b in big:                        # decompress plans write x from the fixed h
            b["pd"] = red.cast_plan([(torch.empty_like(b["x"]), b["h"], n)], DType.FLOAT32)
            b["out"] = b["pd"]._keep[0][0]
            b["pc_h"] = b["pc"]._keep[0][1]
        torch.cuda.synchronize()
    bres = timed_rounds(torch, {
        "plan_compress": (lambda k: big[k]["pc"].compress(), args.inner),
        "single_compress": (lambda k: red.compress_fp16(big[k]["h_out"], big[k]["x"], n,
                                                        DType.FLOAT32), args.inner),
        "plan_decompress": (lambda k: big[k]["pd"].decompress(8), args.inner),
        "single_decompress": (lambda k: red.decompress_fp16(big[k]["out"], big[k]["h"], n,
                                                            DType.FLOAT32, 8), args.inner),
    }, len(big), args)
    for v in bres.values():
        v["roofline_frac"] = round(6 * n / (v["ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
    big_sp = {}
    for d in ("compress", "decompress"):
        sp = max(bres[f"plan_{d}"]["spread_ms"], bres[f"single_{d}"]["spread_ms"])
        big_sp[d] = sp
        gates[f"big_plan_{d}_within_spread_of_single"] = \
            bres[f"plan_{d}"]["ms"] - bres[f"single_{d}"]["ms"] <= sp
    with step("check, one segment", 60):
        b = big[0]
        b["pc"].compress()
        out["bit_equal_one_segment"] = bool(torch.equal(b["pc_h"].view(torch.int16),
                                                        b["h"].view(torch.int16)))
        torch.cuda.synchronize()
    out.update({"big_elems": n, "big": bres, "big_gate_spread_ms": big_sp, "gates": gates})
    for b in big:
        b["pc"].close()
        b["pd"].close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0 if all(gates.values()) else 1


def wire_mode(args) -> int:
    """The bf16 wire against the fp16 wire, alternated in one run."""
    import torch

    from prophet_amd.dtypes import DType
    from prophet_amd.reducer import GpuReducer

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    dev = torch.device("cuda:0")
    F32, WIRES = DType.FLOAT32, {"fp16": (DType.FLOAT16, torch.float16),
                                 "bf16": (DType.BFLOAT16, torch.bfloat16)}
    out = {"tool": "bench_compress", "wire": "bf16", "sets": args.sets, "rounds": args.rounds,
           "inner": args.inner, "device": torch.cuda.get_device_name(0)}
    with step("setup", 120):
        red = GpuReducer(device=0)
        g = torch.Generator(device=dev).manual_seed(3)
        sets = []
        if args.iteration:
            total_bytes, rows = read_table(args.table)
            n = sum(ln // 2 for _, ln in rows)
            for _ in range(args.sets):
                s = {}
                for w, (wd, tdt) in WIRES.items():
                    # a wide arena per wire: each plan writes the one it was built over
                    wide = torch.randn(total_bytes // 2, device=dev, generator=g) * 64
                    half = wide.to(tdt)
                    s[w] = {"wide": wide, "half": half,
                            "plan": red.cast_plan([(wide[o // 2:(o + ln) // 2],
                                                    half[o // 2:(o + ln) // 2], ln // 2)
                                                   for o, ln in rows], F32, wd)}
                sets.append(s)
            out.update({"mode": "iteration", "table": os.path.basename(args.table),
                        "segments": len(rows), "elems": n})
        else:
            n = args.elems
            for _ in range(args.sets):
                x = torch.randn(n, device=dev, generator=g) * 64
                s = {"x": x, "out": torch.empty(n, device=dev)}
                for w, (_, tdt) in WIRES.items():
                    s[w] = {"h": torch.empty(n, dtype=tdt, device=dev), "h2": x.to(tdt)}
                sets.append(s)
            out.update({"mode": "one tensor", "elems": n})
        torch.cuda.synchronize()

    same = {}
    with step("check", 120):
        s = sets[0]
        for w, (wd, tdt) in WIRES.items():
            bits = torch.int16
            if args.iteration:
                a = s[w]
                want = a["wide"].to(tdt)
                a["half"].fill_(7.0)
                a["plan"].compress()
                # the table's segments need not cover the arena: compare where they do
                cover = torch.zeros(a["half"].numel(), dtype=torch.bool, device=dev)
                for o, ln in rows:
                    cover[o // 2:(o + ln) // 2] = True
                same[f"compress_{w}"] = bool(torch.equal(a["half"].view(bits)[cover],
                                                         want.view(bits)[cover]))
                ref = a["half"].clone().div_(8).float()
                a["plan"].decompress(8)
                same[f"decompress_div8_{w}"] = bool(torch.equal(
                    a["wide"].view(torch.int32)[cover], ref.view(torch.int32)[cover]))
                del ref, want, cover
            else:
                red.compress(s[w]["h"], s["x"], n, F32, wd)
                same[f"compress_{w}"] = bool(torch.equal(s[w]["h"].view(bits),
                                                         s["x"].to(tdt).view(bits)))
                red.decompress(s["out"], s[w]["h"], n, F32, wd, 8)
                ref = s[w]["h"].clone().div_(8).float()
                same[f"decompress_div8_{w}"] = bool(torch.equal(s["out"].view(torch.int32),
                                                                ref.view(torch.int32)))
                del ref
        torch.cuda.synchronize()
    out["bit_equal_to_torch_device_cast"] = same

    cands = {}
    for w, (wd, _) in WIRES.items():
        if args.iteration:
            cands[f"compress_{w}"] = (lambda k, w=w: sets[k][w]["plan"].compress(), args.inner)
            cands[f"decompress_{w}"] = (lambda k, w=w: sets[k][w]["plan"].decompress(8),
                                        args.inner)
        else:
            cands[f"compress_{w}"] = (lambda k, w=w, wd=wd: red.compress(
                sets[k][w]["h"], sets[k]["x"], n, F32, wd), args.inner)
            cands[f"decompress_{w}"] = (lambda k, w=w, wd=wd: red.decompress(
                sets[k]["out"], sets[k][w]["h2"], n, F32, wd, 8), args.inner)
    # alternated: compress fp16, compress bf16, decompress fp16, decompress bf16
    order = ["compress_fp16", "compress_bf16", "decompress_fp16", "decompress_bf16"]
    res = timed_rounds(torch, {k: cands[k] for k in order}, len(sets), args)
    for v in res.values():
        v["roofline_frac"] = round(6 * n / (v["ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
    gates, spreads = {}, {}
    for d in ("compress", "decompress"):
        sp = max(res[f"{d}_fp16"]["spread_ms"], res[f"{d}_bf16"]["spread_ms"])
        spreads[d] = sp
        gates[f"{d}_bf16_not_slower_than_fp16"] = \
            res[f"{d}_bf16"]["ms"] - res[f"{d}_fp16"]["ms"] <= sp
    out.update({"results": res, "gate_spread_ms": spreads, "gates": gates})
    if args.iteration:
        for s in sets:
            for w in WIRES:
                s[w]["plan"].close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0 if all(gates.values()) and all(same.values()) else 1


def ef_mode(args) -> int:
    """The error-feedback compress: fused, torch's composition, the plain one."""
    import torch

    from prophet_amd.dtypes import DType
    from prophet_amd.reducer import GpuReducer

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    dev = torch.device("cuda:0")
    F32 = DType.FLOAT32
    wd, tdt = {"fp16": (DType.FLOAT16, torch.float16),
               "bf16": (DType.BFLOAT16, torch.bfloat16)}[args.wire]
    n = args.elems
    out = {"tool": "bench_compress", "mode": "error feedback", "wire": args.wire, "elems": n,
           "sets": args.sets, "rounds": args.rounds, "inner": args.inner,
           "device": torch.cuda.get_device_name(0)}
    with step("setup", 120):
        red = GpuReducer(device=0)
        g = torch.Generator(device=dev).manual_seed(5)
        sets = []
        for _ in range(args.sets):
            x = torch.randn(n, device=dev, generator=g) * 64
            sets.append({"x": x, "r": x * 2.0 ** -12, "h": torch.empty(n, dtype=tdt, device=dev),
                         "c": torch.empty(n, device=dev), "b": torch.empty(n, device=dev)})
        torch.cuda.synchronize()

    def ef_torch(k):
        s = sets[k]
        torch.add(s["x"], s["r"], out=s["c"])
        s["h"].copy_(s["c"])
        s["b"].copy_(s["h"])
        torch.sub(s["c"], s["b"], out=s["r"])

    with step("check", 120):
        s = sets[0]
        r0 = s["r"].clone()
        ef_torch(0)
        want_h, want_r = s["h"].clone(), s["r"].clone()
        s["r"].copy_(r0)
        red.compress_ef(s["h"], s["r"], s["x"], n, F32, wd)
        same = {"wire": bool(torch.equal(s["h"].view(torch.int16), want_h.view(torch.int16))),
                "residual": bool(torch.equal(s["r"].view(torch.int32), want_r.view(torch.int32)))}
        del r0, want_h, want_r
        torch.cuda.synchronize()
    out["bit_equal_to_torch_composition"] = same

    res = timed_rounds(torch, {
        "ef_hip": (lambda k: red.compress_ef(sets[k]["h"], sets[k]["r"], sets[k]["x"], n, F32, wd),
                   args.inner),
        "ef_torch": (ef_torch, args.inner),
        "plain_hip": (lambda k: red.compress(sets[k]["h"], sets[k]["x"], n, F32, wd), args.inner),
    }, len(sets), args)
    for name, per in (("ef_hip", 14), ("ef_torch", 36), ("plain_hip", 6)):
        res[name]["bytes_per_elem"] = per
        res[name]["roofline_frac"] = round(per * n / (res[name]["ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
    sp = max(res["ef_hip"]["spread_ms"], res["ef_torch"]["spread_ms"])
    gates = {"ef_hip_beats_torch_composition": res["ef_torch"]["ms"] - res["ef_hip"]["ms"] > sp}
    out.update({"results": res, "gate_spread_ms": sp,
                "torch_over_hip": round(res["ef_torch"]["ms"] / res["ef_hip"]["ms"], 2),
                "ef_over_plain": round(res["ef_hip"]["ms"] / res["plain_hip"]["ms"], 3)})
    del sets
    torch.cuda.empty_cache()

    total_bytes, rows = read_table(args.table)
    with step("setup, table", 120):
        nelem = sum(ln // 2 for _, ln in rows)
        tsets = []
        for _ in range(args.sets):
            wide = torch.randn(total_bytes // 2, device=dev, generator=g) * 64
            resid = wide * 2.0 ** -12
            half = torch.empty(total_bytes // 2, dtype=tdt, device=dev)
            segs = [(wide[o // 2:(o + ln) // 2], half[o // 2:(o + ln) // 2],
                     resid[o // 2:(o + ln) // 2]) for o, ln in rows]
            tsets.append({"segs": segs, "half": half, "resid": resid,
                          "plan": red.cast_plan([(w, h, w.numel(), q) for w, h, q in segs], F32,
                                                wd)})
        torch.cuda.synchronize()
    with step("check, table", 120):
        s = tsets[0]
        r0 = s["resid"].clone()
        s["plan"].compress()
        got_h, got_r = s["half"].clone(), s["resid"].clone()
        s["resid"].copy_(r0)
        for w, h, q in s["segs"]:
            red.compress_ef(h, q, w, w.numel(), F32, wd)
        cover = torch.zeros(s["half"].numel(), dtype=torch.bool, device=dev)
        for o, ln in rows:
            cover[o // 2:(o + ln) // 2] = True
        out["plan_bit_equal_to_per_segment_calls"] = {
            "wire": bool(torch.equal(got_h.view(torch.int16)[cover],
                                     s["half"].view(torch.int16)[cover])),
            "residual": bool(torch.equal(got_r.view(torch.int32), s["resid"].view(torch.int32)))}
        del r0, got_h, got_r, cover
        torch.cuda.synchronize()

    def loop(k):
        for w, h, q in tsets[k]["segs"]:
            red.compress_ef(h, q, w, w.numel(), F32, wd)

    few = max(1, args.inner // 8)
    tres = timed_rounds(torch, {"loop": (loop, few),
                                "plan": (lambda k: tsets[k]["plan"].compress(), args.inner)},
                        len(tsets), args)
    tsp = max(tres["loop"]["spread_ms"], tres["plan"]["spread_ms"])
    gates["table_plan_beats_loop"] = tres["loop"]["ms"] - tres["plan"]["ms"] > tsp
    tres["plan"]["roofline_frac"] = round(14 * nelem / (tres["plan"]["ms"] * 1e-3)
                                          / HBM_BYTES_PER_S, 4)
    out.update({"table": os.path.basename(args.table), "segments": len(rows),
                "table_elems": nelem, "table_results": tres, "table_gate_spread_ms": tsp,
                "loop_over_plan": round(tres["loop"]["ms"] / tres["plan"]["ms"], 2),
                "gates": gates})
    for s in tsets:
        s["plan"].close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    ok = all(gates.values()) and all(same.values()) and \
        all(out["plan_bit_equal_to_per_segment_calls"].values())
    return 0 if ok else 1


def sr_mode(args) -> int:
    """The stochastic-rounding compress: fused on both wires, a straddling
    base, torch's composition, the plain and the error-feedback compress."""
    import numpy as np
    import torch

    from prophet_amd import sr
    from prophet_amd.dtypes import DType
    from prophet_amd.reducer import GpuReducer, SrKey

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    dev = torch.device("cuda:0")
    F32, F16, BF16 = DType.FLOAT32, DType.FLOAT16, DType.BFLOAT16
    wd = {"fp16": F16, "bf16": BF16}[args.wire]
    n = args.elems
    key = 0x1234
    out = {"tool": "bench_compress", "mode": "stochastic rounding", "wire": args.wire, "elems": n,
           "sets": args.sets, "rounds": args.rounds, "inner": args.inner,
           "device": torch.cuda.get_device_name(0)}
    with step("setup", 120):
        red = GpuReducer(device=0)
        g = torch.Generator(device=dev).manual_seed(5)
        sets = []
        for _ in range(args.sets):
            x = torch.randn(n + 8, device=dev, generator=g) * 64
            h = torch.empty(n + 16, dtype=torch.int16, device=dev)
            sets.append({"x": x[:n], "x1": x[1:1 + n], "h": h[:n], "h1": h[1:1 + n],
                         "r": x[:n] * 2.0 ** -12, "ri": torch.empty(n, dtype=torch.int32, device=dev),
                         "t": torch.empty(n, dtype=torch.int32, device=dev)})
        torch.cuda.synchronize()
    steps = [0]

    def nxt():
        steps[0] += 1
        return steps[0]

    def wire_of(t, w):
        return t.view(torch.float16 if w == F16 else torch.bfloat16)

    def sr_torch(k):
        s = sets[k]
        torch.randint(0, 65536, (n,), out=s["ri"], generator=g)
        torch.add(s["x"].view(torch.int32), s["ri"], out=s["t"])
        s["t"].bitwise_right_shift_(16)
        s["h"].copy_(s["t"])

    with step("check", 120):
        m = min(n, 1 << 20)
        same = {}
        xs = sets[0]["x"][:m].cpu().numpy()
        xs1 = sets[0]["x1"][:m].cpu().numpy()
        for w, name in ((F16, "fp16"), (BF16, "bf16")):
            red.compress_sr(wire_of(sets[0]["h"], w), sets[0]["x"], n, key, 3, w)
            got = sets[0]["h"][:m].cpu().numpy().view(np.uint16)
            same[name] = bool(np.array_equal(got, sr.sr_round(xs, key, 3, name)))
        red.compress_sr(wire_of(sets[0]["h1"], BF16), sets[0]["x1"], n, key, 3, BF16)
        got = sets[0]["h1"][:m].cpu().numpy().view(np.uint16)
        same["bf16_head7"] = bool(np.array_equal(got, sr.sr_round(xs1, key, 3, "bf16")))
        sr_torch(0)
        torch.cuda.synchronize()
    out["bit_equal_to_host_definition"] = same

    res = timed_rounds(torch, {
        "sr_bf16": (lambda k: red.compress_sr(wire_of(sets[k]["h"], BF16), sets[k]["x"], n, key,
                                              nxt(), BF16), args.inner),
        "sr_fp16": (lambda k: red.compress_sr(wire_of(sets[k]["h"], F16), sets[k]["x"], n, key,
                                              nxt(), F16), args.inner),
        "sr_bf16_head7": (lambda k: red.compress_sr(wire_of(sets[k]["h1"], BF16), sets[k]["x1"], n,
                                                    key, nxt(), BF16), args.inner),
        "plain_hip": (lambda k: red.compress(wire_of(sets[k]["h"], wd), sets[k]["x"], n, F32, wd),
                      args.inner),
        "ef_hip": (lambda k: red.compress_ef(wire_of(sets[k]["h"], wd), sets[k]["r"], sets[k]["x"],
                                             n, F32, wd), args.inner),
        "sr_torch": (sr_torch, args.inner),
    }, len(sets), args)
    for name, per in (("sr_bf16", 6), ("sr_fp16", 6), ("sr_bf16_head7", 6), ("plain_hip", 6),
                      ("ef_hip", 14), ("sr_torch", 26)):
        res[name]["bytes_per_elem"] = per
        res[name]["roofline_frac"] = round(per * n / (res[name]["ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
    sp = res["sr_bf16"]["spread_ms"] + res["sr_torch"]["spread_ms"]
    gates = {"sr_hip_beats_torch_composition": res["sr_torch"]["ms"] - res["sr_bf16"]["ms"] > sp}
    psp = max(res["sr_bf16"]["spread_ms"], res["sr_fp16"]["spread_ms"],
              res["plain_hip"]["spread_ms"])
    out.update({"results": res, "gate_spread_sum_ms": round(sp, 5),
                "torch_over_sr": round(res["sr_torch"]["ms"] / res["sr_bf16"]["ms"], 2),
                "sr_bf16_over_plain": round(res["sr_bf16"]["ms"] / res["plain_hip"]["ms"], 3),
                "sr_fp16_over_plain": round(res["sr_fp16"]["ms"] / res["plain_hip"]["ms"], 3),
                "sr_bf16_over_ef": round(res["sr_bf16"]["ms"] / res["ef_hip"]["ms"], 3),
                "head7_over_sr_bf16": round(res["sr_bf16_head7"]["ms"] / res["sr_bf16"]["ms"], 3),
                "within_spreads_of_plain": {
                    w: abs(res[f"sr_{w}"]["ms"] - res["plain_hip"]["ms"]) <= psp
                    for w in ("bf16", "fp16")}})
    del sets
    torch.cuda.empty_cache()

    total_bytes, rows = read_table(args.table)
    tdt = torch.float16 if wd == F16 else torch.bfloat16
    with step("setup, table", 120):
        nelem = sum(ln // 2 for _, ln in rows)
        tsets = []
        for _ in range(args.sets):
            wide = torch.randn(total_bytes // 2, device=dev, generator=g) * 64
            half = torch.empty(total_bytes // 2, dtype=tdt, device=dev)
            segs = [(wide[o // 2:(o + ln) // 2], half[o // 2:(o + ln) // 2], 1000 + i)
                    for i, (o, ln) in enumerate(rows)]
            tsets.append({"segs": segs, "half": half,
                          "plan": red.cast_plan([(w, h, w.numel(), SrKey(k)) for w, h, k in segs],
                                                F32, wd)})
        torch.cuda.synchronize()
    with step("check, table", 120):
        s = tsets[0]
        s["plan"].compress(step=9)
        got_h = s["half"].clone()
        for w, h, k in s["segs"]:
            red.compress_sr(h, w, w.numel(), k, 9, wd)
        cover = torch.zeros(s["half"].numel(), dtype=torch.bool, device=dev)
        for o, ln in rows:
            cover[o // 2:(o + ln) // 2] = True
        out["plan_bit_equal_to_per_segment_calls"] = bool(
            torch.equal(got_h.view(torch.int16)[cover], s["half"].view(torch.int16)[cover]))
        del got_h, cover
        torch.cuda.synchronize()

    def loop(k):
        st = nxt()
        for w, h, kk in tsets[k]["segs"]:
            red.compress_sr(h, w, w.numel(), kk, st, wd)

    few = max(1, args.inner // 8)
    tres = timed_rounds(torch, {"loop": (loop, few),
                                "plan": (lambda k: tsets[k]["plan"].compress(step=nxt()),
                                         args.inner)},
                        len(tsets), args)
    tsp = max(tres["loop"]["spread_ms"], tres["plan"]["spread_ms"])
    gates["table_plan_beats_loop"] = tres["loop"]["ms"] - tres["plan"]["ms"] > tsp
    tres["plan"]["roofline_frac"] = round(6 * nelem / (tres["plan"]["ms"] * 1e-3)
                                          / HBM_BYTES_PER_S, 4)
    out.update({"table": os.path.basename(args.table), "segments": len(rows),
                "table_elems": nelem, "table_results": tres, "table_gate_spread_ms": tsp,
                "loop_over_plan": round(tres["loop"]["ms"] / tres["plan"]["ms"], 2),
                "gates": gates})
    for s in tsets:
        s["plan"].close()
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    ok = all(gates.values()) and all(same.values()) and out["plan_bit_equal_to_per_segment_calls"]
    return 0 if ok else 1


def stats_mode(args) -> int:
    """The decompress with statistics: against the plain decompress, and
    against the plain decompress followed by torch's norm and isfinite."""
    import torch

    from prophet_amd.dtypes import DType
    from prophet_amd.reducer import GpuReducer

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    dev = torch.device("cuda:0")
    F32 = DType.FLOAT32
    wd, tdt = {"fp16": (DType.FLOAT16, torch.float16),
               "bf16": (DType.BFLOAT16, torch.bfloat16)}[args.wire]
    DIV = 8
    out = {"tool": "bench_compress", "mode": "decompress statistics", "wire": args.wire,
           "divisor": DIV, "sets": args.sets, "rounds": args.rounds, "inner": args.inner,
           "device": torch.cuda.get_device_name(0)}
    gates, checks = {}, {}

    def shape(label, nsegs_rows, arena_elems):
        """One shape: ``nsegs_rows`` = (first element, elements) per segment."""
        nelem = sum(n for _, n in nsegs_rows)
        with step(f"setup, {label}", 120):
            g = torch.Generator(device=dev).manual_seed(7)
            sets = []
            for _ in range(args.sets):
                half = (torch.randn(arena_elems, device=dev, generator=g) * 64).to(tdt)
                wide = torch.empty(arena_elems, device=dev)
                outs = [wide[o:o + n] for o, n in nsegs_rows]
                sets.append({"wide": wide, "half": half, "outs": outs,
                             "st": torch.empty(2 * len(outs), dtype=torch.float64, device=dev),
                             "plan": red.cast_plan([(w, half[o:o + n], n)
                                                    for w, (o, n) in zip(outs, nsegs_rows)],
                                                   F32, wd)})
            for s in sets:                       # the first statistics call allocates
                s["plan"].decompress(DIV, stats=s["st"])
            torch.cuda.synchronize()

        def torch_after(k):
            s = sets[k]
            s["plan"].decompress(DIV)
            if len(s["outs"]) == 1:
                nrm = torch.linalg.vector_norm(s["outs"][0])
                return nrm, torch.isfinite(nrm)
            per = torch.stack(torch._foreach_norm(s["outs"]))
            return per.norm(), torch.isfinite(per).logical_not().sum()

        with step(f"check, {label}", 120):
            s = sets[0]
            s["st"].fill_(float("nan"))
            s["plan"].decompress(DIV, stats=s["st"])
            got = s["st"].view(-1, 2)
            ref = torch.stack([w.double().square().sum() for w in s["outs"]])
            tol = torch.tensor([n * 2.0 ** -52 for _, n in nsegs_rows], dtype=torch.float64,
                               device=dev) * ref
            plain = s["wide"].clone()
            s["wide"].fill_(-1.0)
            s["plan"].decompress(DIV)
            checks[label] = {
                "sumsq_within_bound": bool(((got[:, 0] - ref).abs() <= tol).all()),
                "nonfinite_zero": bool((got[:, 1] == 0).all()),
                "bytes_equal_plain": bool(torch.equal(plain.view(torch.int32),
                                                      s["wide"].view(torch.int32))),
                "norm": float(got[:, 0].sum().sqrt()), "torch_norm": float(torch_after(0)[0])}
            del plain, ref
            torch.cuda.synchronize()
        res = timed_rounds(torch, {
            "plan": (lambda k: sets[k]["plan"].decompress(DIV), args.inner),
            "plan_stats": (lambda k: sets[k]["plan"].decompress(DIV, stats=sets[k]["st"]),
                           args.inner),
            "torch": (torch_after, args.inner)}, len(sets), args)
        for name, per in (("plan", 6), ("plan_stats", 6), ("torch", 10)):
            res[name]["bytes_per_elem"] = per
            res[name]["roofline_frac"] = round(per * nelem / (res[name]["ms"] * 1e-3)
                                               / HBM_BYTES_PER_S, 4)
        sp = max(res["plan_stats"]["spread_ms"], res["torch"]["spread_ms"])
        gates[f"{label}_plan_stats_beats_torch"] = res["torch"]["ms"] - res["plan_stats"]["ms"] > sp
        for s in sets:
            s["plan"].close()
        return {"segments": len(nsegs_rows), "elems": nelem, "results": res,
                "gate_spread_ms": sp,
                "plan_stats_over_plan": round(res["plan_stats"]["ms"] / res["plan"]["ms"], 3),
                "torch_over_plan_stats": round(res["torch"]["ms"] / res["plan_stats"]["ms"], 2)}

    with step("init", 60):
        red = GpuReducer(device=0)
    total_bytes, rows = read_table(args.table)
    out["table"] = os.path.basename(args.table)
    out["iteration"] = shape("table", [(o // 2, ln // 2) for o, ln in rows], total_bytes // 2)
    torch.cuda.empty_cache()
    out["big"] = shape("big", [(0, args.elems)], args.elems)
    out.update({"checks": checks, "gates": gates})
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    ok = all(gates.values()) and all(v for c in checks.values() for k, v in c.items()
                                     if isinstance(v, bool))
    return 0 if ok else 1


def clip_mode(args) -> int:
    """Clip by global norm and unscale: measure + record + scaled decompress
    against the statistics decompress followed by torch's multiply, and
    against the plain decompress followed by torch's clip_grad_norm_."""
    import torch

    from prophet_amd.dtypes import DType
    from prophet_amd.reducer import ClipRecord, GpuReducer

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    dev = torch.device("cuda:0")
    F32 = DType.FLOAT32
    wd, tdt = {"fp16": (DType.FLOAT16, torch.float16),
               "bf16": (DType.BFLOAT16, torch.bfloat16)}[args.wire]
    DIV, EPS, INV = 8, 1e-6, 2.0 ** -7
    out = {"tool": "bench_compress", "mode": "clip by global norm", "wire": args.wire,
           "divisor": DIV, "unscale": INV, "sets": args.sets, "rounds": args.rounds,
           "inner": args.inner, "device": torch.cuda.get_device_name(0)}
    gates, checks = {}, {}

    def shape(label, nsegs_rows, arena_elems):
        """One shape: ``nsegs_rows`` = (first element, elements) per segment."""
        nelem = sum(n for _, n in nsegs_rows)
        with step(f"setup, {label}", 120):
            g = torch.Generator(device=dev).manual_seed(7)
            inv = torch.tensor([INV], dtype=torch.float32, device=dev)
            sets = []
            for _ in range(args.sets):
                half = (torch.randn(arena_elems, device=dev, generator=g) * 64).to(tdt)
                wide = torch.empty(arena_elems, device=dev)
                outs = [wide[o:o + n] for o, n in nsegs_rows]
                params = [torch.nn.Parameter(o, requires_grad=True) for o in outs]
                for prm, o in zip(params, outs):
                    prm.grad = o             # clip_grad_norm_ scales the outputs themselves
                sets.append({"wide": wide, "half": half, "outs": outs, "params": params,
                             "st": torch.empty(2 * len(outs), dtype=torch.float64, device=dev),
                             "rec": ClipRecord(dev),
                             "plan": red.cast_plan([(w, half[o:o + n], n)
                                                    for w, (o, n) in zip(outs, nsegs_rows)],
                                                   F32, wd)})
            for s in sets:                       # the first statistics call allocates
                s["plan"].decompress(DIV, stats=s["st"])
            # a max_norm that clips: a third of the unscaled norm
            max_norm = float(sets[0]["st"].view(-1, 2)[:, 0].sum().sqrt()) * INV / 3
            torch.cuda.synchronize()

        def fused(k):
            s = sets[k]
            s["plan"].measure(DIV, stats=s["st"])
            red.clip_record(s["st"], max_norm, EPS, inv, out=s["rec"])
            s["plan"].decompress(DIV, scale=s["rec"].mult)

        def stats_then_torch(k):
            s = sets[k]
            s["plan"].decompress(DIV, stats=s["st"])
            norm = s["st"].view(-1, 2)[:, 0].sum().sqrt() * INV
            coef = torch.clamp(max_norm / (norm + EPS), max=1.0)
            torch._foreach_mul_(s["outs"], (coef * INV).to(torch.float32))

        def torch_all(k):
            s = sets[k]
            s["plan"].decompress(DIV)
            torch.nn.utils.clip_grad_norm_(s["params"], max_norm / INV, foreach=True)

        with step(f"check, {label}", 120):
            s = sets[0]
            s["plan"].decompress(DIV, stats=s["st"])
            want_rows = s["st"].clone()
            plain = s["wide"].clone()
            s["st"].fill_(float("nan"))
            s["wide"].fill_(-1.0)
            fused(0)
            mult = s["rec"].mult.clone()
            ref_norm = float(want_rows.view(-1, 2)[:, 0].sum().sqrt()) * INV
            checks[label] = {
                "rows_equal_stats": bool(torch.equal(want_rows.view(torch.int64),
                                                     s["st"].view(torch.int64))),
                "bytes_equal_mult_times_plain": bool(torch.equal(
                    (plain * mult).view(torch.int32), s["wide"].view(torch.int32))),
                "norm_matches": abs(float(s["rec"].norm) - ref_norm) <= 1e-12 * ref_norm,
                "clips": float(s["rec"].coef) < 1.0,
                "norm": float(s["rec"].norm), "coef": float(s["rec"].coef),
                "mult": float(mult), "max_norm": max_norm}
            del plain, want_rows
            torch.cuda.synchronize()
        res = timed_rounds(torch, {
            "clip_fused": (fused, args.inner),
            "stats_then_torch": (stats_then_torch, args.inner),
            "torch_all": (torch_all, args.inner)}, len(sets), args)
        for name, per in (("clip_fused", 8), ("stats_then_torch", 14), ("torch_all", 18)):
            res[name]["bytes_per_elem"] = per
            res[name]["roofline_frac"] = round(per * nelem / (res[name]["ms"] * 1e-3)
                                               / HBM_BYTES_PER_S, 4)
        other = min(("stats_then_torch", "torch_all"), key=lambda k: res[k]["ms"])
        sp = max(res["clip_fused"]["spread_ms"], res[other]["spread_ms"])
        gates[f"{label}_clip_fused_beats_the_faster_other"] = \
            res[other]["ms"] - res["clip_fused"]["ms"] > sp
        for s in sets:
            s["plan"].close()
        return {"segments": len(nsegs_rows), "elems": nelem, "results": res,
                "faster_other": other, "gate_spread_ms": sp,
                "other_over_clip_fused": round(res[other]["ms"] / res["clip_fused"]["ms"], 3)}

    with step("init", 60):
        red = GpuReducer(device=0)
    total_bytes, rows = read_table(args.table)
    out["table"] = os.path.basename(args.table)
    out["iteration"] = shape("table", [(o // 2, ln // 2) for o, ln in rows], total_bytes // 2)
    torch.cuda.empty_cache()
    out["big"] = shape("big", [(0, args.elems)], args.elems)
    out.update({"checks": checks, "gates": gates})
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    ok = all(gates.values()) and all(v for c in checks.values() for k, v in c.items()
                                     if isinstance(v, bool))
    return 0 if ok else 1


def sgd_mode(args) -> int:
    """The SGD step inside the decompress: measure + record + apply_sgd
    against measure + record + scaled decompress + torch.optim.SGD (fused,
    foreach); and apply_sgd alone against the scaled decompress + the fused
    step.  Every candidate ends with updated parameters and momenta and owns
    its parameters and momenta."""
    import torch

    from prophet_amd.dtypes import DType
    from prophet_amd.reducer import ClipRecord, GpuReducer

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    dev = torch.device("cuda:0")
    F32 = DType.FLOAT32
    wd_id, tdt = {"fp16": (DType.FLOAT16, torch.float16),
                  "bf16": (DType.BFLOAT16, torch.bfloat16)}[args.wire]
    DIV, EPS, INV = 8, 1e-6, 2.0 ** -7
    LR, MU, WD = 1e-3, 0.9, 1e-4
    out = {"tool": "bench_compress", "mode": "sgd step inside the decompress", "wire": args.wire,
           "divisor": DIV, "unscale": INV, "lr": LR, "momentum": MU, "weight_decay": WD,
           "sets": args.sets, "rounds": args.rounds, "inner": args.inner,
           "device": torch.cuda.get_device_name(0)}
    gates, checks = {}, {}

    def shape(label, seg_rows, arena_elems):
        """One shape: ``seg_rows`` = (first element, elements) per segment."""
        nelem = sum(n for _, n in seg_rows)
        with step(f"setup, {label}", 180):
            g = torch.Generator(device=dev).manual_seed(7)
            inv = torch.tensor([INV], dtype=torch.float32, device=dev)
            sets = []
            for _ in range(args.sets):
                half = (torch.randn(arena_elems, device=dev, generator=g) * 64).to(tdt)
                grad = torch.zeros(arena_elems, device=dev)
                p0 = torch.randn(arena_elems, device=dev, generator=g)
                s = {"half": half, "grad": grad, "p0": p0, "rec": ClipRecord(dev),
                     "st": torch.empty(2 * len(seg_rows), dtype=torch.float64, device=dev)}
                cut = lambda t: [t[o:o + n] for o, n in seg_rows]      # noqa: E731
                # apply: its own parameters and momenta
                s["pa"], s["ma"] = p0.clone(), torch.zeros(arena_elems, device=dev)
                s["plain"] = red.cast_plan([(w, h, n) for w, h, (_, n) in
                                            zip(cut(grad), cut(half), seg_rows)], F32, wd_id)
                s["sgd"] = red.sgd_plan([(p, h, n, m) for p, h, m, (_, n) in
                                         zip(cut(s["pa"]), cut(half), cut(s["ma"]), seg_rows)],
                                        wd_id)
                # torch: parameters whose .grad is the decompress's output
                for kind in ("fused", "foreach"):
                    arena = p0.clone()
                    prm = [torch.nn.Parameter(o, requires_grad=True) for o in cut(arena)]
                    for q, o in zip(prm, cut(grad)):
                        q.grad = o
                    s["p_" + kind] = arena
                    s["opt_" + kind] = torch.optim.SGD(prm, lr=LR, momentum=MU, weight_decay=WD,
                                                       nesterov=True, **{kind: True})
                sets.append(s)
            for s in sets:                       # the first statistics call allocates
                s["plain"].measure(DIV, stats=s["st"])
            max_norm = float(sets[0]["st"].view(-1, 2)[:, 0].sum().sqrt()) * INV / 3
            torch.cuda.synchronize()

        def record(s):
            s["plain"].measure(DIV, stats=s["st"])
            red.clip_record(s["st"], max_norm, EPS, inv, out=s["rec"])

        def apply_only(k):
            s = sets[k]
            s["sgd"].apply(DIV, lr=LR, momentum=MU, weight_decay=WD, nesterov=True,
                           record=s["rec"], skip_nonfinite=True)

        def apply(k):
            record(sets[k])
            apply_only(k)

        def scaled_only(kind):
            def run(k):
                s = sets[k]
                s["plain"].decompress(DIV, scale=s["rec"].mult)
                s["opt_" + kind].step()
            return run

        def scaled(kind):
            only = scaled_only(kind)

            def run(k):
                record(sets[k])
                only(k)
            return run

        with step(f"check, {label}", 180):
            s = sets[0]
            record(s)
            s["plain"].decompress(DIV, scale=s["rec"].mult)
            # the definition, one rounding per torch op, from a zero momentum
            gr, p = s["grad"], s["p0"]
            gr = gr + WD * p
            mn = MU * torch.zeros_like(p) + gr
            want_p = p - LR * (gr + MU * mn)
            apply_only(0)
            scaled_only("fused")(0)
            torch.cuda.synchronize()

            def cover(t):
                """The segments' elements of an arena (the table has gaps)."""
                return torch.cat([t[o:o + n] for o, n in seg_rows])
            close = torch.allclose(cover(s["p_fused"]), cover(want_p), rtol=1e-5, atol=1e-6)
            checks[label] = {
                "apply_params_equal_definition": bool(torch.equal(
                    cover(s["pa"]).view(torch.int32), cover(want_p).view(torch.int32))),
                "apply_momenta_equal_definition": bool(torch.equal(
                    cover(s["ma"]).view(torch.int32), cover(mn).view(torch.int32))),
                "torch_fused_close_to_definition": bool(close),
                "found_inf": float(s["rec"].nonfinite), "mult": float(s["rec"].mult),
                "max_norm": max_norm}
            del gr, mn, want_p
            torch.cuda.synchronize()
        res = timed_rounds(torch, {
            "apply": (apply, args.inner),
            "scaled_fused": (scaled("fused"), args.inner),
            "scaled_foreach": (scaled("foreach"), args.inner),
            "apply_only": (apply_only, args.inner),
            "scaled_fused_only": (scaled_only("fused"), args.inner)}, len(sets), args)
        # bytes an element each must move: measure 2, apply 18, scaled decompress 6, step 20
        for name, per in (("apply", 20), ("scaled_fused", 28), ("scaled_foreach", 28),
                          ("apply_only", 18), ("scaled_fused_only", 26)):
            res[name]["bytes_per_elem"] = per
            res[name]["roofline_frac"] = round(per * nelem / (res[name]["ms"] * 1e-3)
                                               / HBM_BYTES_PER_S, 4)
        other = min(("scaled_fused", "scaled_foreach"), key=lambda k: res[k]["ms"])
        sp = max(res["apply"]["spread_ms"], res[other]["spread_ms"])
        gates[f"{label}_apply_beats_the_faster_torch"] = res[other]["ms"] - res["apply"]["ms"] > sp
        for s in sets:
            s["plain"].close()
            s["sgd"].close()
        return {"segments": len(seg_rows), "elems": nelem, "results": res,
                "faster_torch": other, "gate_spread_ms": sp,
                "torch_over_apply": round(res[other]["ms"] / res["apply"]["ms"], 3),
                "only_torch_over_apply": round(res["scaled_fused_only"]["ms"] /
                                               res["apply_only"]["ms"], 3)}

    with step("init", 60):
        red = GpuReducer(device=0)
    total_bytes, rows = read_table(args.table)
    out["table"] = os.path.basename(args.table)
    out["iteration"] = shape("table", [(o // 2, ln // 2) for o, ln in rows], total_bytes // 2)
    torch.cuda.empty_cache()
    out["big"] = shape("big", [(0, args.elems)], args.elems)
    out.update({"checks": checks, "gates": gates})
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    ok = all(gates.values()) and all(v for c in checks.values() for k, v in c.items()
                                     if isinstance(v, bool))
    return 0 if ok else 1


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
