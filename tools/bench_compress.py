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
    p.add_argument("--onebit", action="store_true",
                   help="1-bit sign compression: the three-launch compress against torch's "
                        "add, abs().mean(), where, sub without any packing, and the 8-source "
                        "fold against eight where + add steps on pre-unpacked bool masks; the "
                        "ResNet-50 table and one segment")
    p.add_argument("--onebit-refold", action="store_true",
                   help="the 1-bit server round: the refold plan (fold in registers, finish, "
                        "pack) against the fold plan into a scratch f32 buffer followed by the "
                        "compress plan, 8 sources; the ResNet-50 table and one segment")
    p.add_argument("--mx-refold", action="store_true",
                   help="the block-scaled server round, fp8 and fp4: the one-launch refold plan "
                        "against the fold plan into a scratch f32 buffer followed by the "
                        "compress plan, 8 sources; the ResNet-50 table and one segment")
    p.add_argument("--topk-refold", action="store_true",
                   help="the top-k server round at ratios 0.01 and 0.001: the refold plan (the "
                        "sparse sum in LDS inside the select's first pass) against the fold plan "
                        "into a scratch f32 buffer followed by the compress plan, 8 sources; the "
                        "ResNet-50 table and one segment")
    p.add_argument("--topk", action="store_true",
                   help="top-k sparsification: the radix-select compress against torch's add, "
                        "topk(abs), gather and zero-scatter per tensor, and the 8-source fold "
                        "against eight index_add_ into a zeroed tensor, at ratios 0.01 and "
                        "0.001; the ResNet-50 table and one segment")
    p.add_argument("--mx", action="store_true",
                   help="block-scaled 8- and 4-bit wires: the one-launch compress against "
                        "torch's add, block amax, scale, clamp, float8_e4m3fn cast, widen, "
                        "multiply, subtract per tensor and against the fp16_ef cast plan, and "
                        "the 8-source fold against eight widen-multiply-add steps on "
                        "pre-unpacked codes; the ResNet-50 table and one segment")
    p.add_argument("--mx-sr", action="store_true",
                   help="stateless block-scaled wires, fp8 and fp4, rotated and not: the "
                        "one-launch compress against the mx*_ef compress of the same tensors "
                        "and against torch's block amax, scale, random add and shift (after a "
                        "sign flip and a 32 x 32 Hadamard matmul where rotated), and the "
                        "8-source rotated fold against the mx fold; the ResNet-50 table and one "
                        "segment")
    p.add_argument("--mx-half", action="store_true",
                   help="the block-scaled wires over one bf16 tensor of --elems: mxfp8_ef, "
                        "mxfp8_sr and mxfp4_rht_sr, compress and 8-source fold, against the "
                        "float32 kernel on the upcast tensor and against torch's upcast + "
                        "float32 compress / float32 fold + torch's downcast")
    p.add_argument("--powersgd", action="store_true",
                   help="PowerSGD at rank 4: the four phases and their sum against torch's add, "
                        "matmul, linalg.qr, matmul, mm and sub per tensor; the ResNet-50 table's "
                        "entries that compress, viewed as matrices, and one 4096 x 16384 matrix")
    args = p.parse_args()
    if args.powersgd:
        return powersgd_mode(args)
    if args.mx_half:
        return mx_half_mode(args)
    if args.mx:
        return mx_mode(args)
    if args.mx_sr:
        return mx_sr_mode(args)
    if args.topk_refold:
        return topk_refold_mode(args)
    if args.topk:
        return topk_mode(args)
    if args.onebit_refold:
        return onebit_refold_mode(args)
    if args.mx_refold:
        return mx_refold_mode(args)
    if args.onebit:
        return onebit_mode(args)
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


def onebit_mode(args) -> int:
    """1-bit sign compression, the --sgd protocol.  The
    compress (accumulate, finish, pack) against torch's composition of the same
    arithmetic per tensor with NO packing — add, abs().mean(), where, sub —
    which favours torch; the 8-source fold against eight where + add steps per
    tensor on bool masks unpacked ahead of time, which favours torch again."""
    import torch

    from prophet_amd import onebit
    from prophet_amd.reducer import GpuReducer

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    dev = torch.device("cuda:0")
    NSRC = 8
    out = {"tool": "bench_compress", "mode": "onebit_ef compress and fold", "nsrc": NSRC,
           "sets": args.sets, "rounds": args.rounds, "inner": args.inner,
           "device": torch.cuda.get_device_name(0)}
    gates, checks = {}, {}

    def shape(label, seg_rows, arena_elems):
        nelem = sum(n for _, n in seg_rows)
        cut = lambda t: [t[o:o + n] for o, n in seg_rows]      # noqa: E731
        pay_off, at = [], 0
        for _, n in seg_rows:                    # 16-byte aligned payloads in one arena
            pay_off.append(at)
            at += (onebit.payload_bytes(n) + 15) & ~15
        pcut = lambda t: [t[o:o + onebit.payload_bytes(n)]     # noqa: E731
                          for o, (_, n) in zip(pay_off, seg_rows)]
        shifts = torch.arange(8, device=dev, dtype=torch.uint8)

        def unpack(p, n):
            """The n sign bits of a device payload as a bool tensor."""
            return ((p[16:].unsqueeze(1) >> shifts) & 1).reshape(-1)[:n].bool()

        with step(f"setup, {label}", 180):
            g = torch.Generator(device=dev).manual_seed(7)
            sets = []
            for _ in range(args.sets):
                s = {"g": torch.randn(arena_elems, device=dev, generator=g),
                     "r": torch.zeros(arena_elems, device=dev),
                     "rt": torch.zeros(arena_elems, device=dev),
                     "out": torch.empty(arena_elems, device=dev),
                     "out_t": torch.empty(arena_elems, device=dev),
                     "payc": torch.empty(at, dtype=torch.uint8, device=dev),
                     "pay": [torch.empty(at, dtype=torch.uint8, device=dev) for _ in range(NSRC)]}
                s["comp"] = red.onebit_plan(list(zip(cut(s["g"]), cut(s["r"]), pcut(s["payc"]),
                                                     [n for _, n in seg_rows])))
                # the fold's sources: the compress of NSRC different gradients
                for k in range(NSRC):
                    gk = torch.randn(arena_elems, device=dev, generator=g) * (k + 1)
                    pl = red.onebit_plan(list(zip(cut(gk), cut(s["rt"]), pcut(s["pay"][k]),
                                                  [n for _, n in seg_rows])))
                    pl.compress()
                    pl.close()
                    s["rt"].zero_()
                s["fold"] = red.onebit_fold_plan(
                    [(o, [pcut(s["pay"][k])[i] for k in range(NSRC)], n)
                     for i, (o, (_, n)) in enumerate(zip(cut(s["out"]), seg_rows))], NSRC)
                s["masks"] = [[unpack(p, n) for p, (_, n) in zip(pcut(s["pay"][k]), seg_rows)]
                              for k in range(NSRC)]
                s["scales"] = [[p[:4].view(torch.float32).clone() for p in pcut(s["pay"][k])]
                               for k in range(NSRC)]
                sets.append(s)
            torch.cuda.synchronize()

        def compress(k):
            sets[k]["comp"].compress()

        def torch_compress(k):
            s = sets[k]
            for gi, ri in zip(cut(s["g"]), cut(s["rt"])):
                c = gi + ri
                scale = c.abs().mean()
                torch.sub(c, torch.where(c < 0, -scale, scale), out=ri)

        def fold(k):
            sets[k]["fold"].launch(1)

        def torch_fold(k):
            s = sets[k]
            for i, o in enumerate(cut(s["out_t"])):
                sc = s["scales"][0][i]
                torch.where(s["masks"][0][i], -sc, sc, out=o)
                for j in range(1, NSRC):
                    sc = s["scales"][j][i]
                    o.add_(torch.where(s["masks"][j][i], -sc, sc))

        with step(f"check, {label}", 180):
            s = sets[0]
            torch_compress(0)
            s["rt"].zero_()
            compress(0)
            fold(0)
            torch_fold(0)
            torch.cuda.synchronize()
            bits_ok = all(bool(torch.equal(unpack(p, n), gi < 0))      # r was zero: c = g
                          for p, gi, (_, n) in zip(pcut(s["payc"]), cut(s["g"]), seg_rows))
            fold_ok = all(bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))
                          for a, b in zip(cut(s["out"]), cut(s["out_t"])))
            checks[label] = {"compress_bits_equal_torch_signs": bits_ok,
                             "fold_equals_torch_left_fold": fold_ok}
            s["r"].zero_()
        res = timed_rounds(torch, {"compress": (compress, args.inner),
                                   "torch_compress": (torch_compress, args.inner),
                                   "fold": (fold, args.inner),
                                   "torch_fold": (torch_fold, args.inner)}, len(sets), args)
        # bytes an element the design moves: 12 + 8.125 (compress), 4 + N / 8 (fold)
        for name, per in (("compress", 20.125), ("fold", 4 + NSRC / 8)):
            res[name]["bytes_per_elem"] = per
            res[name]["roofline_frac"] = round(per * nelem / (res[name]["ms"] * 1e-3)
                                               / HBM_BYTES_PER_S, 4)
        for ours, theirs in (("compress", "torch_compress"), ("fold", "torch_fold")):
            sp = max(res[ours]["spread_ms"], res[theirs]["spread_ms"])
            gates[f"{label}_{ours}_beats_torch"] = res[theirs]["ms"] - res[ours]["ms"] > sp
        for s in sets:
            s["comp"].close()
            s["fold"].close()
        return {"segments": len(seg_rows), "elems": nelem, "results": res}

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
    return 0 if all(gates.values()) and all(v for c in checks.values() for v in c.values()) else 1


def topk_mode(args) -> int:
    """Top-k sparsification, the --onebit protocol, at ratios
    0.01 and 0.001.  The compress against torch's composition per tensor — add
    into the residual, topk(abs), gather, zero-scatter — which leaves its
    entries unsorted and so favours torch; the 8-source fold against eight
    index_add_ per tensor into a zeroed tensor, on int64 indices converted
    ahead of time, which favours torch again.  Before timing, ours is compared
    with prophet_amd/topk.py byte for byte, and with torch by the sorted
    magnitudes it selected (torch's tie order differs, the multiset does not)."""
    import numpy as np
    import torch

    from prophet_amd import topk
    from prophet_amd.reducer import GpuReducer

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    dev = torch.device("cuda:0")
    NSRC = 8
    out = {"tool": "bench_compress", "mode": "topk_ef compress and fold", "nsrc": NSRC,
           "sets": args.sets, "rounds": args.rounds, "inner": args.inner,
           "device": torch.cuda.get_device_name(0)}
    gates, checks = {}, {}

    def shape(label, ratio, seg_rows, arena_elems):
        nelem = sum(n for _, n in seg_rows)
        counts = [n for _, n in seg_rows]
        kk = [topk.k_for(n, ratio) for n in counts]
        cut = lambda t: [t[o:o + n] for o, n in seg_rows]      # noqa: E731
        pay_off, at = [], 0
        for k in kk:                             # 16-byte aligned payloads in one arena
            pay_off.append(at)
            at += (topk.payload_bytes(k) + 15) & ~15
        pcut = lambda t: [t[o:o + topk.payload_bytes(k)]       # noqa: E731
                          for o, k in zip(pay_off, kk)]

        def entries(p, k):
            return p[16:16 + 4 * k].view(torch.int32), p[16 + 4 * k:16 + 8 * k].view(torch.float32)

        with step(f"setup, {label}", 300):
            g = torch.Generator(device=dev).manual_seed(7)
            sets = []
            for _ in range(args.sets):
                s = {"g": torch.randn(arena_elems, device=dev, generator=g),
                     "r": torch.zeros(arena_elems, device=dev),
                     "rt": torch.zeros(arena_elems, device=dev),
                     "out": torch.empty(arena_elems, device=dev),
                     "out_t": torch.empty(arena_elems, device=dev),
                     "payc": torch.empty(at, dtype=torch.uint8, device=dev),
                     "pay": [torch.empty(at, dtype=torch.uint8, device=dev) for _ in range(NSRC)]}
                s["comp"] = red.topk_plan(list(zip(cut(s["g"]), cut(s["r"]), pcut(s["payc"]),
                                                   counts, kk)))
                # the fold's sources: the compress of NSRC different gradients
                for j in range(NSRC):
                    gj = torch.randn(arena_elems, device=dev, generator=g) * (j + 1)
                    pl = red.topk_plan(list(zip(cut(gj), cut(s["rt"]), pcut(s["pay"][j]),
                                                counts, kk)))
                    pl.compress()
                    pl.close()
                    s["rt"].zero_()
                s["fold"] = red.topk_fold_plan(
                    [(o, [pcut(s["pay"][j])[i] for j in range(NSRC)], n, k)
                     for i, (o, n, k) in enumerate(zip(cut(s["out"]), counts, kk))], NSRC)
                s["idx"] = [[entries(p, k)[0].long() for p, k in zip(pcut(s["pay"][j]), kk)]
                            for j in range(NSRC)]
                s["val"] = [[entries(p, k)[1] for p, k in zip(pcut(s["pay"][j]), kk)]
                            for j in range(NSRC)]
                s["tv"] = [None] * len(kk)       # what torch's compress selected
                sets.append(s)
            torch.cuda.synchronize()

        def compress(i):
            sets[i]["comp"].compress()

        def torch_compress(i):
            s = sets[i]
            for t, (gi, ri, k) in enumerate(zip(cut(s["g"]), cut(s["rt"]), kk)):
                torch.add(gi, ri, out=ri)
                idx = torch.topk(ri.abs(), k, sorted=False).indices
                s["tv"][t] = ri[idx]
                ri[idx] = 0.0

        def fold(i):
            sets[i]["fold"].launch(1)

        def torch_fold(i):
            s = sets[i]
            s["out_t"].zero_()
            for t, o in enumerate(cut(s["out_t"])):
                for j in range(NSRC):
                    o.index_add_(0, s["idx"][j][t], s["val"][j][t])

        with step(f"check, {label}", 600):
            s = sets[0]
            torch_compress(0)
            compress(0)
            fold(0)
            torch_fold(0)
            torch.cuda.synchronize()
            gh, rh, ph = s["g"].cpu().numpy(), s["r"].cpu().numpy(), s["payc"].cpu().numpy()
            srch = [x.cpu().numpy() for x in s["pay"]]
            oh = s["out"].cpu().numpy()
            def_ok = fold_ok = torch_ok = True
            for t, ((o, n), po, k) in enumerate(zip(seg_rows, pay_off, kk)):
                nb = topk.payload_bytes(k)
                pay, rn = topk.compress(gh[o:o + n], np.zeros(n, np.float32), k)
                def_ok = def_ok and np.array_equal(ph[po:po + nb], pay) and \
                    np.array_equal(rh[o:o + n].view(np.uint32), rn.view(np.uint32))
                fold_ok = fold_ok and np.array_equal(
                    oh[o:o + n].view(np.uint32),
                    topk.fold([x[po:po + nb] for x in srch], n, 1, k).view(np.uint32))
                ours = np.sort(np.abs(topk.entries(pay, k)[1]))
                torch_ok = torch_ok and np.array_equal(
                    ours, np.sort(np.abs(s["tv"][t].cpu().numpy())))
            fold_t = all(bool(torch.equal(a, b)) for a, b in zip(cut(s["out"]), cut(s["out_t"])))
            checks[label] = {"compress_equals_definition": bool(def_ok),
                             "fold_equals_definition": bool(fold_ok),
                             "compress_selects_torch_magnitudes": bool(torch_ok),
                             "fold_equals_torch_index_add": fold_t}
            s["r"].zero_()
            s["rt"].zero_()
        res = timed_rounds(torch, {"compress": (compress, args.inner),
                                   "torch_compress": (torch_compress, args.inner),
                                   "fold": (fold, args.inner),
                                   "torch_fold": (torch_fold, args.inner)}, len(sets), args)
        # bytes an element the design moves: ACCUMULATE 12, REFINE 4 + 4, COUNT 4,
        # COMPACT 4 and per entry 8 of payload and at most 16 of r'; the fold 4
        # and 8 an entry a source
        kn = sum(kk) / nelem
        for name, per in (("compress", 28 + 24 * kn), ("fold", 4 + 8 * NSRC * kn)):
            res[name]["bytes_per_elem"] = round(per, 4)
            res[name]["roofline_frac"] = round(per * nelem / (res[name]["ms"] * 1e-3)
                                               / HBM_BYTES_PER_S, 4)
        for ours, theirs in (("compress", "torch_compress"), ("fold", "torch_fold")):
            sp = max(res[ours]["spread_ms"], res[theirs]["spread_ms"])
            gates[f"{label}_{ours}_beats_torch"] = res[theirs]["ms"] - res[ours]["ms"] > sp
        for s in sets:
            s["comp"].close()
            s["fold"].close()
        return {"segments": len(seg_rows), "elems": nelem, "k": sum(kk), "results": res}

    with step("init", 60):
        red = GpuReducer(device=0)
    total_bytes, rows = read_table(args.table)
    out["table"] = os.path.basename(args.table)
    for ratio in (0.01, 0.001):
        out[f"iteration_{ratio}"] = shape(f"table_{ratio}", ratio,
                                          [(o // 2, ln // 2) for o, ln in rows], total_bytes // 2)
        torch.cuda.empty_cache()
        out[f"big_{ratio}"] = shape(f"big_{ratio}", ratio, [(0, args.elems)], args.elems)
        torch.cuda.empty_cache()
    out.update({"checks": checks, "gates": gates})
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0 if all(gates.values()) and all(v for c in checks.values() for v in c.values()) else 1


def mx_mode(args) -> int:
    """The block-scaled wires, the --onebit protocol, fp8 and
    fp4.  The compress against two yardsticks: torch's composition per tensor —
    add into the residual, view as blocks of 32, integer-key amax, scale, clamp,
    cast to float8_e4m3fn, widen, multiply, subtract — on tensors padded to
    whole blocks ahead of time, which favours torch; and the fp16_ef cast plan
    of the same tensors, 14 B an element against 13.03 and 12.53.  The 8-source
    fold against eight widen-multiply-add steps per tensor on codes and scales
    unpacked ahead of time.  torch has no e2m1 cast: its fp4 column is the same
    composition with emax 2, max 6 and the e4m3 cast.  Before timing, ours is
    compared with prophet_amd/mx.py byte for byte: payloads, residuals, folds."""
    import numpy as np
    import torch

    from prophet_amd import mx
    from prophet_amd.dtypes import DType
    from prophet_amd.reducer import GpuReducer

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    dev = torch.device("cuda:0")
    NSRC = 8
    out = {"tool": "bench_compress", "mode": "mxfp8_ef / mxfp4_ef compress and fold",
           "nsrc": NSRC, "sets": args.sets, "rounds": args.rounds, "inner": args.inner,
           "device": torch.cuda.get_device_name(0)}
    gates, checks = {}, {}

    def shape(label, fmt, seg_rows, arena_elems):
        bits, emax, vmax = mx.bits_of(fmt), mx._FORMATS[fmt][1], mx._FORMATS[fmt][2]
        nelem = sum(n for _, n in seg_rows)
        counts = [n for _, n in seg_rows]
        cut = lambda t: [t[o:o + n] for o, n in seg_rows]      # noqa: E731
        pay_off, pad_off, at, pat = [], [], 0, 0
        for n in counts:                         # 16-byte aligned payloads in one arena
            pay_off.append(at)
            pad_off.append(pat)
            at += mx.payload_bytes(n, fmt)
            pat += -(-n // 32) * 32              # torch's copies: whole blocks a tensor
        pcut = lambda t: [t[o:o + mx.payload_bytes(n, fmt)]    # noqa: E731
                          for o, n in zip(pay_off, counts)]
        padcut = lambda t: [t[o:o + -(-n // 32) * 32].view(-1, 32)   # noqa: E731
                            for o, n in zip(pad_off, counts)]

        with step(f"setup, {label}", 300):
            g = torch.Generator(device=dev).manual_seed(13)
            sets = []
            for _ in range(args.sets):
                s = {"g": torch.randn(arena_elems, device=dev, generator=g),
                     "r": torch.zeros(arena_elems, device=dev),
                     "r16": torch.zeros(arena_elems, device=dev),
                     "h16": torch.empty(arena_elems, dtype=torch.float16, device=dev),
                     "out": torch.empty(arena_elems, device=dev),
                     "gt": torch.zeros(pat, device=dev), "rt": torch.zeros(pat, device=dev),
                     "out_t": torch.empty(pat, device=dev),
                     "payc": torch.empty(at, dtype=torch.uint8, device=dev),
                     "pay": [torch.empty(at, dtype=torch.uint8, device=dev) for _ in range(NSRC)]}
                for a, b in zip(padcut(s["gt"]), cut(s["g"])):
                    a.view(-1)[:b.numel()].copy_(b)
                s["comp"] = red.mx_plan(list(zip(cut(s["g"]), cut(s["r"]), pcut(s["payc"]),
                                                 counts)), fmt)
                s["ef16"] = red.cast_plan([(w, h, w.numel(), q) for w, h, q in
                                           zip(cut(s["g"]), cut(s["h16"]), cut(s["r16"]))],
                                          DType.FLOAT32, DType.FLOAT16)
                # the fold's sources: the compress of NSRC different gradients
                s["tq"], s["tx"] = [], []
                for j in range(NSRC):
                    gj = torch.randn(arena_elems, device=dev, generator=g) * (j + 1)
                    pl = red.mx_plan(list(zip(cut(gj), cut(s["out"]), pcut(s["pay"][j]), counts)),
                                     fmt)
                    s["out"].zero_()
                    pl.compress()
                    pl.close()
                    # torch's sources: e4m3 codes and f32 scales of the same gradients
                    tq, tx = [], []
                    for b in cut(gj):
                        pb = torch.zeros(-(-b.numel() // 32) * 32, device=dev)
                        pb[:b.numel()] = b
                        pb = pb.view(-1, 32)
                        X = (((pb.view(torch.int32) & 0x7fffffff).amax(1) >> 23) - emax).clamp_(0)
                        v = (pb * ((254 - X) << 23).view(torch.float32)[:, None]).clamp_(-vmax, vmax)
                        tq.append(v.to(torch.float8_e4m3fn))
                        tx.append((X << 23).view(torch.float32)[:, None].clone())
                    s["tq"].append(tq)
                    s["tx"].append(tx)
                    del gj
                s["fold"] = red.mx_fold_plan(
                    [(o, [pcut(s["pay"][j])[i] for j in range(NSRC)], n)
                     for i, (o, n) in enumerate(zip(cut(s["out"]), counts))], NSRC, fmt)
                sets.append(s)
            torch.cuda.synchronize()

        def compress(i):
            sets[i]["comp"].compress()

        def fp16_ef(i):
            sets[i]["ef16"].compress()

        def torch_compress(i):
            s = sets[i]
            for gb, rb in zip(padcut(s["gt"]), padcut(s["rt"])):
                torch.add(gb, rb, out=rb)
                X = (((rb.view(torch.int32) & 0x7fffffff).amax(1) >> 23) - emax).clamp_(0)
                v = (rb * ((254 - X) << 23).view(torch.float32)[:, None]).clamp_(-vmax, vmax)
                q = v.to(torch.float8_e4m3fn)
                rb.sub_(q.float() * (X << 23).view(torch.float32)[:, None])

        def fold(i):
            sets[i]["fold"].launch(1)

        def torch_fold(i):
            s = sets[i]
            for t, o in enumerate(padcut(s["out_t"])):
                torch.mul(s["tq"][0][t].float(), s["tx"][0][t], out=o)
                for j in range(1, NSRC):
                    o.add_(s["tq"][j][t].float() * s["tx"][j][t])

        with step(f"check, {label}", 900):
            s = sets[0]
            torch_compress(0)
            fp16_ef(0)
            compress(0)
            fold(0)
            torch_fold(0)
            torch.cuda.synchronize()
            gh, rh, ph = s["g"].cpu().numpy(), s["r"].cpu().numpy(), s["payc"].cpu().numpy()
            srch = [x.cpu().numpy() for x in s["pay"]]
            oh = s["out"].cpu().numpy()
            def_ok = fold_ok = True
            for (o, n), po in zip(seg_rows, pay_off):
                nb = mx.payload_bytes(n, fmt)
                pay, rn = mx.compress(gh[o:o + n], np.zeros(n, np.float32), fmt)
                def_ok = def_ok and np.array_equal(ph[po:po + nb], pay) and \
                    np.array_equal(rh[o:o + n].view(np.uint32), rn.view(np.uint32))
                fold_ok = fold_ok and np.array_equal(
                    oh[o:o + n].view(np.uint32),
                    mx.fold([x[po:po + nb] for x in srch], n, fmt, 1).view(np.uint32))
            checks[label] = {"compress_equals_definition": bool(def_ok),
                             "fold_equals_definition": bool(fold_ok)}
            if fmt == "fp8":                     # torch's columns compute the same values there
                checks[label]["torch_residual_equals_ours"] = all(
                    bool(torch.equal(a.reshape(-1)[:b.numel()], b))
                    for a, b in zip(padcut(s["rt"]), cut(s["r"])))
                checks[label]["torch_fold_equals_ours"] = all(
                    bool(torch.equal(a.reshape(-1)[:b.numel()], b))
                    for a, b in zip(padcut(s["out_t"]), cut(s["out"])))
            del gh, rh, ph, srch, oh
            for name in ("r", "rt", "r16"):
                s[name].zero_()
        res = timed_rounds(torch, {"compress": (compress, args.inner),
                                   "torch_compress": (torch_compress, args.inner),
                                   "fp16_ef": (fp16_ef, args.inner),
                                   "fold": (fold, args.inner),
                                   "torch_fold": (torch_fold, args.inner)}, len(sets), args)
        # bytes an element the designs move: 12 + bits / 8 + 1 / 32 (compress),
        # 14 (fp16_ef), 4 + N (bits / 8 + 1 / 32) (fold)
        wire = bits / 8 + 1 / 32
        for name, per in (("compress", 12 + wire), ("fp16_ef", 14.0), ("fold", 4 + NSRC * wire)):
            res[name]["bytes_per_elem"] = round(per, 4)
            res[name]["roofline_frac"] = round(per * nelem / (res[name]["ms"] * 1e-3)
                                               / HBM_BYTES_PER_S, 4)
        for ours, theirs in (("compress", "torch_compress"), ("fold", "torch_fold")):
            sp = max(res[ours]["spread_ms"], res[theirs]["spread_ms"])
            gates[f"{label}_{ours}_beats_torch"] = res[theirs]["ms"] - res[ours]["ms"] > sp
        sp = max(res["compress"]["spread_ms"], res["fp16_ef"]["spread_ms"])
        gates[f"{label}_compress_not_slower_than_fp16_ef"] = \
            res["compress"]["ms"] - res["fp16_ef"]["ms"] <= sp
        for s in sets:
            for name in ("comp", "fold", "ef16"):
                s[name].close()
        return {"segments": len(seg_rows), "elems": nelem, "results": res}

    with step("init", 60):
        red = GpuReducer(device=0)
    total_bytes, rows = read_table(args.table)
    out["table"] = os.path.basename(args.table)
    for fmt in ("fp8", "fp4"):
        out[f"iteration_{fmt}"] = shape(f"table_{fmt}", fmt,
                                        [(o // 2, ln // 2) for o, ln in rows], total_bytes // 2)
        torch.cuda.empty_cache()
        out[f"big_{fmt}"] = shape(f"big_{fmt}", fmt, [(0, args.elems)], args.elems)
        torch.cuda.empty_cache()
    out.update({"checks": checks, "gates": gates})
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0 if all(gates.values()) and all(v for c in checks.values() for v in c.values()) else 1


def mx_sr_mode(args) -> int:
    """The stateless block-scaled wires, the --mx protocol:
    fp8 and fp4, rotated and not.  The compress against the mx*_ef compress of
    the same tensors in the same run (4 + bits / 8 + 1 / 32 bytes an element
    against 12 + ...) and against torch's composition per tensor on tensors
    padded to whole blocks ahead of time — integer-key amax, the bumped scale,
    multiply, random 16 bits added to the magnitude's bits, shift, cast to
    uint8 (the normal-range path only, torch.randint for the bits), after a
    sign flip and a matmul with the 32 x 32 Hadamard matrix where rotated: all
    of which favours torch.  The 8-source rotated fold against the mx fold of
    the same payloads, which moves the same bytes.  Before timing, ours is
    compared with prophet_amd/mx_sr.py byte for byte: payloads and folds."""
    import numpy as np
    import torch

    from prophet_amd import mx, mx_sr
    from prophet_amd.reducer import GpuReducer

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    dev = torch.device("cuda:0")
    NSRC, STEP = 8, 3
    out = {"tool": "bench_compress", "mode": "mxfp8/4_sr and _rht_sr compress and fold",
           "nsrc": NSRC, "sets": args.sets, "rounds": args.rounds, "inner": args.inner,
           "device": torch.cuda.get_device_name(0)}
    gates, checks = {}, {}
    had = torch.tensor([[(-1.0) ** bin(i & j).count("1") for j in range(32)] for i in range(32)],
                       device=dev)

    def shape(label, fmt, rot, seg_rows, arena_elems):
        bits, emax, _, mbits, bias = mx._FORMATS[fmt]
        mant = 0x600000 if fmt == "fp8" else 0x400000
        nelem, counts = sum(n for _, n in seg_rows), [n for _, n in seg_rows]
        cut = lambda t: [t[o:o + n] for o, n in seg_rows]      # noqa: E731
        pay_off, pad_off, at, pat = [], [], 0, 0
        for n in counts:
            pay_off.append(at)
            pad_off.append(pat)
            at += mx.payload_bytes(n, fmt)
            pat += -(-n // 32) * 32
        pcut = lambda t: [t[o:o + mx.payload_bytes(n, fmt)]    # noqa: E731
                          for o, n in zip(pay_off, counts)]
        padcut = lambda t: [t[o:o + -(-n // 32) * 32].view(-1, 32)   # noqa: E731
                            for o, n in zip(pad_off, counts)]
        keys = [(1000 + i, 77 + i) for i in range(len(counts))]

        with step(f"setup, {label}", 300):
            g = torch.Generator(device=dev).manual_seed(13)
            sets = []
            for _ in range(args.sets):
                s = {"g": torch.randn(arena_elems, device=dev, generator=g),
                     "r": torch.zeros(arena_elems, device=dev),
                     "out": torch.empty(arena_elems, device=dev),
                     "gt": torch.zeros(pat, device=dev),
                     "qt": torch.empty(pat, dtype=torch.uint8, device=dev),
                     "sign": torch.randint(0, 2, (pat,), device=dev, generator=g).float() * 2 - 1,
                     "payc": torch.empty(at, dtype=torch.uint8, device=dev),
                     "paye": torch.empty(at, dtype=torch.uint8, device=dev),
                     "pay": [torch.empty(at, dtype=torch.uint8, device=dev) for _ in range(NSRC)]}
                for a, b in zip(padcut(s["gt"]), cut(s["g"])):
                    a.view(-1)[:b.numel()].copy_(b)
                s["comp"] = red.mx_sr_plan([(w, p, n, k, rk) for w, p, n, (k, rk) in
                                            zip(cut(s["g"]), pcut(s["payc"]), counts, keys)],
                                           fmt, rot)
                s["ef"] = red.mx_plan(list(zip(cut(s["g"]), cut(s["r"]), pcut(s["paye"]), counts)),
                                      fmt)
                for j in range(NSRC):                # the fold's sources: NSRC other gradients
                    gj = torch.randn(arena_elems, device=dev, generator=g) * (j + 1)
                    pl = red.mx_sr_plan([(w, p, n, k + j, rk) for w, p, n, (k, rk) in
                                         zip(cut(gj), pcut(s["pay"][j]), counts, keys)], fmt, rot)
                    pl.compress(STEP)
                    pl.close()
                    del gj
                srcs = [(o, [pcut(s["pay"][j])[i] for j in range(NSRC)], n)
                        for i, (o, n) in enumerate(zip(cut(s["out"]), counts))]
                s["mxfold"] = red.mx_fold_plan(srcs, NSRC, fmt)
                s["fold"] = red.mx_rht_fold_plan(
                    [(o, ps, n, rk) for (o, ps, n), (_, rk) in zip(srcs, keys)], NSRC, fmt) \
                    if rot else s["mxfold"]
                sets.append(s)
            torch.cuda.synchronize()

        def compress(i):
            sets[i]["comp"].compress(STEP)

        def mx_ef(i):
            sets[i]["ef"].compress()

        def torch_compress(i):
            s = sets[i]
            for gb, sb, qb in zip(padcut(s["gt"]), padcut(s["sign"]), padcut(s["qt"])):
                c = torch.mm(gb * sb, had) if rot else gb
                K = (c.view(torch.int32) & 0x7fffffff).amax(1)
                X = ((K >> 23) - emax + ((K & 0x7fffff) > mant)).clamp_(0)
                v = (c * ((254 - X) << 23).view(torch.float32)[:, None]).view(torch.int32)
                t = ((v & 0x7fffffff) >> (7 - mbits)) - (((127 - bias) << mbits) << 16)
                t = (t + torch.randint(0, 65536, t.shape, device=dev, dtype=torch.int32)) >> 16
                torch.bitwise_or(t.clamp_(0), (v >> 31) & (1 << (bits - 1)), out=t)
                qb.copy_(t)

        def fold(i):
            if rot:
                sets[i]["fold"].launch(1, STEP)
            else:
                sets[i]["fold"].launch(1)

        def mx_fold(i):
            sets[i]["mxfold"].launch(1)

        with step(f"check, {label}", 1500):
            s = sets[0]
            torch_compress(0)
            compress(0)
            fold(0)
            torch.cuda.synchronize()
            gh, ph, oh = s["g"].cpu().numpy(), s["payc"].cpu().numpy(), s["out"].cpu().numpy()
            srch = [x.cpu().numpy() for x in s["pay"]]
            def_ok = fold_ok = True
            for (o, n), po, (k, rk) in zip(seg_rows, pay_off, keys):
                nb = mx.payload_bytes(n, fmt)
                def_ok = def_ok and np.array_equal(
                    ph[po:po + nb], mx_sr.compress(gh[o:o + n], fmt, k, STEP, rot, rk))
                fold_ok = fold_ok and np.array_equal(
                    oh[o:o + n].view(np.uint32),
                    mx_sr.fold([x[po:po + nb] for x in srch], n, fmt, 1, rot, rk, STEP)
                    .view(np.uint32))
            checks[label] = {"compress_equals_definition": bool(def_ok),
                             "fold_equals_definition": bool(fold_ok)}
            del gh, ph, oh, srch
        cands = {"compress": (compress, args.inner), "mx_ef_compress": (mx_ef, args.inner),
                 "torch_compress": (torch_compress, args.inner), "fold": (fold, args.inner)}
        if rot:
            cands["mx_fold"] = (mx_fold, args.inner)
        res = timed_rounds(torch, cands, len(sets), args)
        wire = bits / 8 + 1 / 32
        for name, per in (("compress", 4 + wire), ("mx_ef_compress", 12 + wire),
                          ("fold", 4 + NSRC * wire)):
            res[name]["bytes_per_elem"] = round(per, 4)
            res[name]["roofline_frac"] = round(per * nelem / (res[name]["ms"] * 1e-3)
                                               / HBM_BYTES_PER_S, 4)
        res["compress"]["ratio_to_mx_ef"] = round(res["compress"]["ms"]
                                                  / res["mx_ef_compress"]["ms"], 4)
        sp = max(res["compress"]["spread_ms"], res["torch_compress"]["spread_ms"])
        gates[f"{label}_compress_beats_torch"] = \
            res["torch_compress"]["ms"] - res["compress"]["ms"] > sp
        for s in sets:
            for name in ("comp", "ef", "mxfold") + (("fold",) if rot else ()):
                s[name].close()
        return {"segments": len(seg_rows), "elems": nelem, "results": res}

    with step("init", 60):
        red = GpuReducer(device=0)
    total_bytes, rows = read_table(args.table)
    out["table"] = os.path.basename(args.table)
    for fmt in ("fp8", "fp4"):
        for rot in (False, True):
            tag = fmt + ("_rht" if rot else "")
            out[f"iteration_{tag}"] = shape(f"table_{tag}", fmt, rot,
                                            [(o // 2, ln // 2) for o, ln in rows],
                                            total_bytes // 2)
            torch.cuda.empty_cache()
            out[f"big_{tag}"] = shape(f"big_{tag}", fmt, rot, [(0, args.elems)], args.elems)
            torch.cuda.empty_cache()
    out.update({"checks": checks, "gates": gates})
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0 if all(gates.values()) and all(v for c in checks.values() for v in c.values()) else 1


def mx_half_mode(args) -> int:
    """The block-scaled wires over a bf16 tensor: mxfp8_ef,
    mxfp8_sr and mxfp4_rht_sr, the compress and the 8-source fold of one
    ``--elems`` tensor, each against two things in the same run: the float32
    kernel on the upcast tensor, and today's route for a half tensor — torch's
    upcast into a ready float32 buffer and the float32 compress; the float32
    fold into a float32 buffer and torch's downcast.  Before timing, the bf16
    compress's payload is compared with the float32 one's byte for byte, and
    the bf16 fold's output with the downcast float32 fold."""
    import torch

    from prophet_amd import mx
    from prophet_amd.dtypes import DType
    from prophet_amd.reducer import GpuReducer

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    dev = torch.device("cuda:0")
    NSRC, STEP, KEY, RK, n = 8, 3, 1000, 77, args.elems
    BF = DType.BFLOAT16
    out = {"tool": "bench_compress", "mode": "block-scaled wires over a bf16 tensor",
           "elems": n, "nsrc": NSRC, "sets": args.sets, "rounds": args.rounds,
           "inner": args.inner, "device": torch.cuda.get_device_name(0)}
    checks = {}

    def wire(label, fmt, kind):
        nb = mx.payload_bytes(n, fmt)
        rot = kind == "rht"

        def comp_plan(g, r, p, dtype):
            if kind == "ef":
                return red.mx_plan([(g, r, p, n)], fmt, dtype)
            return red.mx_sr_plan([(g, p, n, KEY, RK)], fmt, rot, dtype)

        def fold_plan(o, ps, dtype):
            if rot:
                return red.mx_rht_fold_plan([(o, ps, n, RK)], NSRC, fmt, dtype)
            return red.mx_fold_plan([(o, ps, n)], NSRC, fmt, dtype)

        with step(f"setup, {label}", 300):
            gen = torch.Generator(device=dev).manual_seed(13)
            sets = []
            for _ in range(args.sets):
                s = {"g16": torch.randn(n, device=dev, generator=gen).bfloat16(),
                     "r16": torch.zeros(n, device=dev), "r32": torch.zeros(n, device=dev),
                     "tmp": torch.empty(n, device=dev),
                     "o16": torch.empty(n, dtype=torch.bfloat16, device=dev),
                     "o32": torch.empty(n, device=dev),
                     "p16": torch.empty(nb, dtype=torch.uint8, device=dev),
                     "p32": torch.empty(nb, dtype=torch.uint8, device=dev),
                     "src": [torch.empty(nb, dtype=torch.uint8, device=dev) for _ in range(NSRC)]}
                s["g32"] = s["g16"].float()
                s["c16"] = comp_plan(s["g16"], s["r16"], s["p16"], BF)
                s["c32"] = comp_plan(s["g32"], s["r32"], s["p32"], DType.FLOAT32)
                s["ctoday"] = comp_plan(s["tmp"], s["r32"], s["p32"], DType.FLOAT32)
                for j in range(NSRC):                # the fold's sources: NSRC other gradients
                    gj = (torch.randn(n, device=dev, generator=gen) * (j + 1)).bfloat16()
                    pl = comp_plan(gj, s["tmp"].zero_(), s["src"][j], BF)
                    pl.compress(*((STEP,) if kind != "ef" else ()))
                    pl.close()
                    del gj
                s["f16"] = fold_plan(s["o16"], s["src"], BF)
                s["f32"] = fold_plan(s["o32"], s["src"], DType.FLOAT32)
                s["ftoday"] = fold_plan(s["tmp"], s["src"], DType.FLOAT32)
                sets.append(s)
            torch.cuda.synchronize()

        run = (lambda pl: pl.compress()) if kind == "ef" else (lambda pl: pl.compress(STEP))
        launch = (lambda pl: pl.launch(1, STEP)) if rot else (lambda pl: pl.launch(1))

        def today_compress(i):
            sets[i]["tmp"].copy_(sets[i]["g16"])
            run(sets[i]["ctoday"])

        def today_fold(i):
            launch(sets[i]["ftoday"])
            sets[i]["o16"].copy_(sets[i]["tmp"])

        with step(f"check, {label}", 300):
            s = sets[0]
            run(s["c16"])
            run(s["c32"])
            launch(s["f16"])
            launch(s["ftoday"])
            torch.cuda.synchronize()
            checks[label] = {
                "payload_equals_float32_route": bool(torch.equal(s["p16"], s["p32"])),
                "fold_equals_downcast_float32_fold": bool(torch.equal(
                    s["o16"].view(torch.int16), s["tmp"].bfloat16().view(torch.int16)))}
            for t in ("r16", "r32"):
                s[t].zero_()
        cands = {"compress": (lambda i: run(sets[i]["c16"]), args.inner),
                 "f32_compress": (lambda i: run(sets[i]["c32"]), args.inner),
                 "today_compress": (today_compress, args.inner),
                 "fold": (lambda i: launch(sets[i]["f16"]), args.inner),
                 "f32_fold": (lambda i: launch(sets[i]["f32"]), args.inner),
                 "today_fold": (today_fold, args.inner)}
        res = timed_rounds(torch, cands, len(sets), args)
        w, side = mx.bits_of(fmt) / 8 + 1 / 32, 8 if kind == "ef" else 0
        for name, per in (("compress", 2 + side + w), ("f32_compress", 4 + side + w),
                          ("fold", 2 + NSRC * w), ("f32_fold", 4 + NSRC * w)):
            res[name]["bytes_per_elem"] = round(per, 4)
            res[name]["roofline_frac"] = round(per * n / (res[name]["ms"] * 1e-3)
                                               / HBM_BYTES_PER_S, 4)
        for what in ("compress", "fold"):
            res[what]["speedup_over_today"] = round(res[f"today_{what}"]["ms"] / res[what]["ms"], 4)
            res[what]["ratio_to_f32"] = round(res[what]["ms"] / res[f"f32_{what}"]["ms"], 4)
        for s in sets:
            for name in ("c16", "c32", "ctoday", "f16", "f32", "ftoday"):
                s[name].close()
        return res

    with step("init", 60):
        red = GpuReducer(device=0)
    for label, fmt, kind in (("mxfp8_ef", "fp8", "ef"), ("mxfp8_sr", "fp8", "sr"),
                             ("mxfp4_rht_sr", "fp4", "rht")):
        out[label] = wire(label, fmt, kind)
        torch.cuda.empty_cache()
    out["checks"] = checks
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0 if all(v for c in checks.values() for v in c.values()) else 1


def powersgd_mode(args) -> int:
    """PowerSGD, the --onebit protocol, rank 4.  The table
    holds flat sizes, so an entry of N >= 4096 elements is viewed as the n x N / n
    matrix with n the largest power of two that divides N, n <= 512 and n n <= N
    (64 x 147, 512 x 1152, 512 x 4000, ...); the shorter entries are the vectors
    of the model and do not compress.  Each phase is timed on its own and the
    four are added; torch's column is the same iteration per tensor: add, matmul,
    linalg.qr, matmul, mm, sub.  Before timing, one iteration from a zero residual:
    out against torch's out, and R against g - out byte for byte."""
    import torch

    from prophet_amd.reducer import GpuReducer

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    dev = torch.device("cuda:0")
    RANK = 4
    out = {"tool": "bench_compress", "mode": "powersgd_ef phases", "rank": RANK,
           "sets": args.sets, "rounds": args.rounds, "inner": args.inner,
           "device": torch.cuda.get_device_name(0)}
    gates, checks = {}, {}
    PHASES = ("project_p", "orthogonalize", "project_q", "finish")

    def shape(label, mats):
        nelem = sum(n * m for n, m in mats)
        small = sum((n + m) * RANK for n, m in mats)

        def cut(t, sizes):                       # consecutive 2-d views of a flat arena
            views, at = [], 0
            for rows, cols in sizes:
                views.append(t[at:at + rows * cols].view(rows, cols))
                at += rows * cols
            return views
        with step(f"setup, {label}", 300):
            gen = torch.Generator(device=dev).manual_seed(13)
            sets = []
            for _ in range(args.sets):
                s = {k: cut(torch.zeros(nelem, device=dev), mats) for k in ("R", "Rt", "out", "out_t")}
                s["g"] = cut(torch.randn(nelem, device=dev, generator=gen), mats)
                s["Q"] = cut(torch.randn(small, device=dev, generator=gen),
                             [(m, RANK) for _, m in mats])
                s["P"] = cut(torch.zeros(small, device=dev), [(n, RANK) for n, _ in mats])
                s["Qn"] = cut(torch.zeros(small, device=dev), [(m, RANK) for _, m in mats])
                s["Pt"], s["Qt"] = [torch.zeros_like(x) for x in s["P"]], \
                    [torch.zeros_like(x) for x in s["Qn"]]
                s["plan"] = red.powersgd_plan(
                    [(g, r, pp, q, qn, o, n, m) for g, r, pp, q, qn, o, (n, m) in
                     zip(s["g"], s["R"], s["P"], s["Q"], s["Qn"], s["out"], mats)], RANK)
                sets.append(s)
            torch.cuda.synchronize()

        def torch_iteration(i):
            s = sets[i]
            for g, r, q, pt, qt, o in zip(s["g"], s["Rt"], s["Q"], s["Pt"], s["Qt"], s["out_t"]):
                torch.add(g, r, out=r)
                torch.matmul(r, q, out=pt)
                ph = torch.linalg.qr(pt)[0]
                torch.matmul(r.t(), ph, out=qt)
                torch.mm(ph, qt.t(), out=o)
                r.sub_(o)

        with step(f"check, {label}", 300):
            s = sets[0]
            s["plan"].project_p()
            torch_iteration(0)
            for name in PHASES[1:]:
                getattr(s["plan"], name)()
            torch.cuda.synchronize()
            close = True
            for g, r, o, ot in zip(s["g"], s["R"], s["out"], s["out_t"]):   # R was 0: M is g
                close = close and bool((o - ot).abs().max() <= 1e-3 * g.abs().max())
                close = close and bool(torch.equal(r, torch.where(torch.isfinite(o), g - o, 0.0)))
            checks[label] = {"out_close_to_torch_and_residual_is_g_minus_out": close}
            for name in ("R", "Rt"):
                for x in s[name]:
                    x.zero_()
        cands = {name: ((lambda i, name=name: getattr(sets[i]["plan"], name)()), args.inner)
                 for name in PHASES}
        cands["torch_iteration"] = (torch_iteration, max(1, args.inner // 4))
        res = timed_rounds(torch, cands, len(sets), args)
        total = sum(res[name]["ms"] for name in PHASES)
        spread = sum(res[name]["spread_ms"] for name in PHASES)
        res["sum_of_phases"] = {"ms": round(total, 5), "spread_ms": round(spread, 5),
                                "bytes_per_elem": 28.0,
                                "roofline_frac": round(28.0 * nelem / (total * 1e-3)
                                                       / HBM_BYTES_PER_S, 4),
                                "torch_over_ours": round(res["torch_iteration"]["ms"] / total, 2)}
        for name, per in (("project_p", 12.0), ("project_q", 4.0), ("finish", 12.0)):
            res[name]["roofline_frac"] = round(per * nelem / (res[name]["ms"] * 1e-3)
                                               / HBM_BYTES_PER_S, 4)
        gates[f"{label}_sum_beats_torch"] = \
            res["torch_iteration"]["ms"] - total > max(spread, res["torch_iteration"]["spread_ms"])
        for s in sets:
            s["plan"].close()
        return {"segments": len(mats), "elems": nelem, "wire_floats": small, "results": res}

    def matrix_of(nelem):
        n = 512
        while nelem % n or n * n > nelem:
            n //= 2
        return n, nelem // n

    with step("init", 60):
        red = GpuReducer(device=0)
    _, rows = read_table(args.table)
    out["table"] = os.path.basename(args.table)
    out["iteration"] = shape("table", [matrix_of(ln // 2) for _, ln in rows if ln // 2 >= 4096])
    torch.cuda.empty_cache()
    out["big"] = shape("big", [(4096, 16384)])
    out.update({"checks": checks, "gates": gates})
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    return 0 if all(gates.values()) and all(v for c in checks.values() for v in c.values()) else 1


def onebit_refold_mode(args) -> int:
    """The 1-bit server round, the --onebit protocol.  The
    refold plan against what it replaces: the 8-source fold plan into a scratch
    f32 buffer, then the compress plan of that buffer against the residual.
    Before timing both produce the same output payload and residual bytes (the
    sources' scales are powers of two there, so the f64 sum has one value in
    any order)."""
    import torch

    from prophet_amd import onebit
    from prophet_amd.reducer import GpuReducer

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    dev = torch.device("cuda:0")
    NSRC = 8
    out = {"tool": "bench_compress", "mode": "onebit_ef refold against fold + compress",
           "nsrc": NSRC, "sets": args.sets, "rounds": args.rounds, "inner": args.inner,
           "device": torch.cuda.get_device_name(0)}
    gates, checks = {}, {}

    def shape(label, seg_rows, arena_elems):
        nelem = sum(n for _, n in seg_rows)
        counts = [n for _, n in seg_rows]
        cut = lambda t: [t[o:o + n] for o, n in seg_rows]      # noqa: E731
        pay_off, at = [], 0
        for n in counts:                         # 16-byte aligned payloads in one arena
            pay_off.append(at)
            at += (onebit.payload_bytes(n) + 15) & ~15
        pcut = lambda t: [t[o:o + onebit.payload_bytes(n)]     # noqa: E731
                          for o, n in zip(pay_off, counts)]
        with step(f"setup, {label}", 180):
            g = torch.Generator(device=dev).manual_seed(11)
            sets = []
            for _ in range(args.sets):
                s = {"r": torch.zeros(arena_elems, device=dev),        # the refold's residual
                     "rc": torch.zeros(arena_elems, device=dev),       # the composition's
                     "sum": torch.empty(arena_elems, device=dev),      # its scratch f32 sum
                     "zero": torch.zeros(arena_elems, device=dev),
                     "out": torch.empty(at, dtype=torch.uint8, device=dev),
                     "outc": torch.empty(at, dtype=torch.uint8, device=dev),
                     "pay": [torch.empty(at, dtype=torch.uint8, device=dev) for _ in range(NSRC)]}
                for k in range(NSRC):            # the sources: NSRC compressed gradients
                    gk = torch.randn(arena_elems, device=dev, generator=g)
                    pl = red.onebit_plan(list(zip(cut(gk), cut(s["zero"]), pcut(s["pay"][k]),
                                                  counts)))
                    pl.compress()
                    pl.close()
                    s["zero"].zero_()
                    for p in pcut(s["pay"][k]):  # a power of two for a scale
                        p[:4].view(torch.float32).fill_(2.0 ** (k % 3))
                rows = [[pcut(s["pay"][k])[i] for k in range(NSRC)] for i in range(len(counts))]
                s["refold"] = red.onebit_refold_plan(
                    list(zip(rows, cut(s["r"]), pcut(s["out"]), counts)), NSRC)
                s["fold"] = red.onebit_fold_plan(list(zip(cut(s["sum"]), rows, counts)), NSRC)
                s["comp"] = red.onebit_plan(list(zip(cut(s["sum"]), cut(s["rc"]), pcut(s["outc"]),
                                                     counts)))
                del s["zero"]
                sets.append(s)
            torch.cuda.synchronize()

        def refold(k):
            sets[k]["refold"].launch()

        def composed(k):
            sets[k]["fold"].launch(1)
            sets[k]["comp"].compress()

        with step(f"check, {label}", 180):
            s = sets[0]
            for _ in range(2):                   # twice: the residual carries
                refold(0)
                composed(0)
            torch.cuda.synchronize()
            checks[label] = {
                "payload_bytes_equal": all(bool(torch.equal(a, b)) for a, b in
                                           zip(pcut(s["out"]), pcut(s["outc"]))),
                "residual_bytes_equal": bool(torch.equal(s["r"].view(torch.int32),
                                                         s["rc"].view(torch.int32)))}
        res = timed_rounds(torch, {"refold": (refold, args.inner),
                                   "composed": (composed, args.inner)}, len(sets), args)
        # bytes an element the designs move: 16.125 + N / 8 against 24.125 + N / 8
        for name, per in (("refold", 16.125 + NSRC / 8), ("composed", 24.125 + NSRC / 8)):
            res[name]["bytes_per_elem"] = per
            res[name]["roofline_frac"] = round(per * nelem / (res[name]["ms"] * 1e-3)
                                               / HBM_BYTES_PER_S, 4)
        sp = max(res["refold"]["spread_ms"], res["composed"]["spread_ms"])
        gates[f"{label}_refold_beats_composed"] = res["composed"]["ms"] - res["refold"]["ms"] > sp
        for s in sets:
            for name in ("refold", "fold", "comp"):
                s[name].close()
        return {"segments": len(seg_rows), "elems": nelem, "results": res}

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
    # the gate that must hold is the one-tensor shape's; the table's is reported
    ok = gates["big_refold_beats_composed"] and all(v for c in checks.values()
                                                    for v in c.values())
    return 0 if ok else 1


def mx_refold_mode(args) -> int:
    """The block-scaled server round, the --onebit-refold
    protocol for both formats.  The refold plan against what it replaces on the
    same commit: the 8-source fold plan into a scratch f32 buffer, then the
    compress plan of that buffer against the residual.  Before timing both
    produce the same output payload and residual bytes, twice over so that the
    residual carries."""
    import torch

    from prophet_amd import mx
    from prophet_amd.reducer import GpuReducer

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    dev = torch.device("cuda:0")
    NSRC = 8
    out = {"tool": "bench_compress", "mode": "mx*_ef refold against fold + compress",
           "nsrc": NSRC, "sets": args.sets, "rounds": args.rounds, "inner": args.inner,
           "device": torch.cuda.get_device_name(0)}
    gates, checks = {}, {}

    def shape(label, fmt, seg_rows, arena_elems):
        nelem = sum(n for _, n in seg_rows)
        counts = [n for _, n in seg_rows]
        cut = lambda t: [t[o:o + n] for o, n in seg_rows]      # noqa: E731
        pay_off, at = [], 0
        for n in counts:                         # payloads are whole multiples of 16 bytes
            pay_off.append(at)
            at += mx.payload_bytes(n, fmt)
        pcut = lambda t: [t[o:o + mx.payload_bytes(n, fmt)]    # noqa: E731
                          for o, n in zip(pay_off, counts)]
        with step(f"setup, {label}", 180):
            g = torch.Generator(device=dev).manual_seed(11)
            sets = []
            for _ in range(args.sets):
                s = {"r": torch.zeros(arena_elems, device=dev),        # the refold's residual
                     "rc": torch.zeros(arena_elems, device=dev),       # the composition's
                     "sum": torch.empty(arena_elems, device=dev),      # its scratch f32 sum
                     "zero": torch.zeros(arena_elems, device=dev),
                     "out": torch.empty(at, dtype=torch.uint8, device=dev),
                     "outc": torch.empty(at, dtype=torch.uint8, device=dev),
                     "pay": [torch.empty(at, dtype=torch.uint8, device=dev) for _ in range(NSRC)]}
                for k in range(NSRC):            # the sources: NSRC compressed gradients
                    gk = torch.randn(arena_elems, device=dev, generator=g)
                    pl = red.mx_plan(list(zip(cut(gk), cut(s["zero"]), pcut(s["pay"][k]), counts)),
                                     fmt)
                    pl.compress()
                    pl.close()
                    s["zero"].zero_()
                rows = [[pcut(s["pay"][k])[i] for k in range(NSRC)] for i in range(len(counts))]
                s["refold"] = red.mx_refold_plan(
                    list(zip(rows, cut(s["r"]), pcut(s["out"]), counts)), NSRC, fmt)
                s["fold"] = red.mx_fold_plan(list(zip(cut(s["sum"]), rows, counts)), NSRC, fmt)
                s["comp"] = red.mx_plan(list(zip(cut(s["sum"]), cut(s["rc"]), pcut(s["outc"]),
                                                 counts)), fmt)
                del s["zero"]
                sets.append(s)
            torch.cuda.synchronize()

        def refold(k):
            sets[k]["refold"].launch()

        def composed(k):
            sets[k]["fold"].launch(1)
            sets[k]["comp"].compress()

        with step(f"check, {label}", 180):
            s = sets[0]
            for _ in range(2):                   # twice: the residual carries
                refold(0)
                composed(0)
            torch.cuda.synchronize()
            checks[label] = {
                "payload_bytes_equal": all(bool(torch.equal(a, b)) for a, b in
                                           zip(pcut(s["out"]), pcut(s["outc"]))),
                "residual_bytes_equal": bool(torch.equal(s["r"].view(torch.int32),
                                                         s["rc"].view(torch.int32)))}
        res = timed_rounds(torch, {"refold": (refold, args.inner),
                                   "composed": (composed, args.inner)}, len(sets), args)
        # bytes an element the designs move, from the definition: a payload is
        # bits / 8 + 1 / 32; the refold reads N of them and r, writes one and r';
        # the pair also writes and reads the f32 sum
        pay = mx.bits_of(fmt) / 8 + 1 / 32
        for name, per in (("refold", 8 + (NSRC + 1) * pay), ("composed", 16 + (NSRC + 1) * pay)):
            res[name]["bytes_per_elem"] = per
            res[name]["roofline_frac"] = round(per * nelem / (res[name]["ms"] * 1e-3)
                                               / HBM_BYTES_PER_S, 4)
        sp = max(res["refold"]["spread_ms"], res["composed"]["spread_ms"])
        gates[f"{label}_refold_beats_composed"] = res["composed"]["ms"] - res["refold"]["ms"] > sp
        for s in sets:
            for name in ("refold", "fold", "comp"):
                s[name].close()
        return {"fmt": fmt, "segments": len(seg_rows), "elems": nelem, "results": res}

    with step("init", 60):
        red = GpuReducer(device=0)
    total_bytes, rows = read_table(args.table)
    out["table"] = os.path.basename(args.table)
    for fmt in ("fp8", "fp4"):
        out[f"iteration_{fmt}"] = shape(f"table_{fmt}", fmt,
                                        [(o // 2, ln // 2) for o, ln in rows], total_bytes // 2)
        torch.cuda.empty_cache()
        out[f"big_{fmt}"] = shape(f"big_{fmt}", fmt, [(0, args.elems)], args.elems)
        torch.cuda.empty_cache()
    out.update({"checks": checks, "gates": gates})
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    # the bytes must agree; the ratio is a recorded fact
    return 0 if all(v for c in checks.values() for v in c.values()) else 1


def topk_refold_mode(args) -> int:
    """The top-k server round, the --mx-refold protocol at
    ratios 0.01 and 0.001.  The refold plan against what it replaces on the same
    commit: the 8-source fold plan into a scratch f32 buffer, then the compress
    plan of that buffer against the residual.  Before timing both produce the
    same output payload and residual bytes, twice over so that the residual
    carries."""
    import torch

    from prophet_amd import topk
    from prophet_amd.reducer import GpuReducer

    if not torch.cuda.is_available():
        print(json.dumps({"error": "no GPU: nothing is measured without one"}))
        return 2
    dev = torch.device("cuda:0")
    NSRC = 8
    out = {"tool": "bench_compress", "mode": "topk_ef refold against fold + compress",
           "nsrc": NSRC, "sets": args.sets, "rounds": args.rounds, "inner": args.inner,
           "device": torch.cuda.get_device_name(0)}
    gates, checks = {}, {}

    def shape(label, ratio, seg_rows, arena_elems):
        counts = [n for _, n in seg_rows]
        ks = [topk.k_for(n, ratio) for n in counts]
        nelem, ktot = sum(counts), sum(ks)
        cut = lambda t: [t[o:o + n] for o, n in seg_rows]      # noqa: E731
        pay_off, at = [], 0
        for k in ks:                             # every payload at a 16-byte boundary
            pay_off.append(at)
            at += (topk.payload_bytes(k) + 15) & ~15
        pcut = lambda t: [t[o:o + topk.payload_bytes(k)]       # noqa: E731
                          for o, k in zip(pay_off, ks)]
        with step(f"setup, {label}", 180):
            g = torch.Generator(device=dev).manual_seed(11)
            sets = []
            for _ in range(args.sets):
                s = {"r": torch.zeros(arena_elems, device=dev),        # the refold's residual
                     "rc": torch.zeros(arena_elems, device=dev),       # the composition's
                     "sum": torch.empty(arena_elems, device=dev),      # its scratch f32 sum
                     "zero": torch.zeros(arena_elems, device=dev),
                     "out": torch.empty(at, dtype=torch.uint8, device=dev),
                     "outc": torch.empty(at, dtype=torch.uint8, device=dev),
                     "pay": [torch.empty(at, dtype=torch.uint8, device=dev) for _ in range(NSRC)]}
                for j in range(NSRC):            # the sources: NSRC compressed gradients
                    gj = torch.randn(arena_elems, device=dev, generator=g)
                    pl = red.topk_plan(list(zip(cut(gj), cut(s["zero"]), pcut(s["pay"][j]),
                                                counts, ks)))
                    pl.compress()
                    pl.close()
                    s["zero"].zero_()
                rows = [[pcut(s["pay"][j])[i] for j in range(NSRC)] for i in range(len(counts))]
                s["refold"] = red.topk_refold_plan(
                    list(zip(rows, cut(s["r"]), pcut(s["out"]), counts, ks)), NSRC)
                s["fold"] = red.topk_fold_plan(list(zip(cut(s["sum"]), rows, counts, ks)), NSRC)
                s["comp"] = red.topk_plan(list(zip(cut(s["sum"]), cut(s["rc"]), pcut(s["outc"]),
                                                   counts, ks)))
                del s["zero"]
                sets.append(s)
            torch.cuda.synchronize()

        def refold(i):
            sets[i]["refold"].launch()

        def composed(i):
            sets[i]["fold"].launch(1)
            sets[i]["comp"].compress()

        with step(f"check, {label}", 180):
            s = sets[0]
            for _ in range(2):                   # twice: the residual carries
                refold(0)
                composed(0)
            torch.cuda.synchronize()
            checks[label] = {
                "payload_bytes_equal": all(bool(torch.equal(a, b)) for a, b in
                                           zip(pcut(s["out"]), pcut(s["outc"]))),
                "residual_bytes_equal": bool(torch.equal(s["r"].view(torch.int32),
                                                         s["rc"].view(torch.int32)))}
        res = timed_rounds(torch, {"refold": (refold, args.inner),
                                   "composed": (composed, args.inner)}, len(sets), args)
        # bytes an element the designs move, from the definition: the first pass
        # reads N payloads and r and writes c, REFINE 1, REFINE 2, COUNT and
        # COMPACT read c once each, COMPACT writes one payload and the k changed
        # residual vectors (16 bytes each at these ratios); the pair also writes
        # and reads the f32 sum
        sparse = (8 * NSRC + 24) * ktot / nelem
        for name, per in (("refold", 24 + sparse), ("composed", 32 + sparse)):
            res[name]["bytes_per_elem"] = round(per, 4)
            res[name]["roofline_frac"] = round(per * nelem / (res[name]["ms"] * 1e-3)
                                               / HBM_BYTES_PER_S, 4)
        res["ratio_refold_over_composed"] = round(res["refold"]["ms"] / res["composed"]["ms"], 4)
        sp = max(res["refold"]["spread_ms"], res["composed"]["spread_ms"])
        gates[f"{label}_refold_beats_composed"] = res["composed"]["ms"] - res["refold"]["ms"] > sp
        for s in sets:
            for name in ("refold", "fold", "comp"):
                s[name].close()
        return {"ratio": ratio, "segments": len(seg_rows), "elems": nelem, "entries": ktot,
                "results": res}

    with step("init", 60):
        red = GpuReducer(device=0)
    total_bytes, rows = read_table(args.table)
    out["table"] = os.path.basename(args.table)
    for ratio in (0.01, 0.001):
        out[f"iteration_{ratio}"] = shape(f"table_{ratio}", ratio,
                                          [(o // 2, ln // 2) for o, ln in rows], total_bytes // 2)
        torch.cuda.empty_cache()
        out[f"big_{ratio}"] = shape(f"big_{ratio}", ratio, [(0, args.elems)], args.elems)
        torch.cuda.empty_cache()
    out.update({"checks": checks, "gates": gates})
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    # the bytes must agree; the ratio is a recorded fact
    return 0 if all(v for c in checks.values() for v in c.values()) else 1


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
