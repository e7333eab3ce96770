// The cast plan's kernel and launch over the per-tile code of
// bpsr_cast_impl.h.  A template on the rounding scheme S and with it the narrow
// (wire) format, so that each (scheme, wire format) instantiates it in a
// translation unit of its own (plain: bpsr_k_cast_plan.hip,
// bpsr_k_cast_plan_bf16.hip; error feedback: bpsr_k_cast_ef*.hip; stochastic
// rounding: bpsr_k_cast_sr*.hip).  What a plan is and how a record is read:
// bpsr_k_cast_plan.hip.  The decompress has a STATS variant that also reports
// each segment's sum of squares and non-finite count, a
// MEASURE variant that reports the same and stores nothing, and a SCALED
// variant that multiplies every value it writes.
#pragma once

#include "bpsr_cast_impl.h"

namespace bpsr {

// One wave's statistics of one record (byteps_reduce_cast_plan_decompress_stats):
// kBlock / 64 of them a record, 64 bytes, in a plan-owned array indexed by
// (record, wave) that cast_stats_finish_kernel adds up per segment.
struct StatPart {
  double sumsq;
  uint64_t nonfinite;
};
static_assert(sizeof(StatPart) * (kBlock / 64) == 64, "64 bytes of partials a record");

// The STATS variant's kernel argument: the plan and the partials.
template <class S>
struct PlanStats {
  typename S::Plan plan;
  StatPart* part;
};
// The SCALED variant's: the plan and the device-resident multiplier.
template <class S>
struct PlanScaled {
  typename S::Plan plan;
  const float* mult;
};
template <class P>
__device__ __forceinline__ const P& plan_of(const P& a) { return a; }
template <class S>
__device__ __forceinline__ const typename S::Plan& plan_of(const PlanStats<S>& a) {
  return a.plan;
}
template <class S>
__device__ __forceinline__ const typename S::Plan& plan_of(const PlanScaled<S>& a) {
  return a.plan;
}

// The decompress's compile-time variants: its kernel argument and the
// accumulator the tiles take (bpsr_cast_impl.h).
enum { kPlanPlain = 0, kPlanStats = 1, kPlanMeasure = 2, kPlanScaled = 3 };
template <class S, int MODE>
struct PlanMode {
  using Arg = typename S::Plan;
  using Acc = StatNone;
};
template <class S>
struct PlanMode<S, kPlanStats> {
  using Arg = PlanStats<S>;
  using Acc = StatAcc;
};
template <class S>
struct PlanMode<S, kPlanMeasure> {
  using Arg = PlanStats<S>;
  using Acc = StatMeasure;
};
template <class S>
struct PlanMode<S, kPlanScaled> {
  using Arg = PlanScaled<S>;
  using Acc = StatScale;
};

// Lane l's 64 bits from lane `from / 4`: the two halves through ds_bpermute.
__device__ __forceinline__ uint64_t stat_from_lane(uint64_t b, int from) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)(uint32_t)b);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)(uint32_t)(b >> 32));
  return ((uint64_t)hi << 32) | lo;
}

// The sums over the wave's 64 lanes, in every lane: six butterfly steps.  All
// 64 lanes active.  The pairing is fixed, so the same lane values give the
// same bits.  C: uint32_t (a record's count) or uint64_t (a segment's).
template <class C>
__device__ __forceinline__ void stat_wave_sum(double& x, C& n) {
  const int l = (int)(threadIdx.x & 63);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const int from = (l ^ m) * 4;
    x += bitcast<double>(stat_from_lane(bitcast<uint64_t>(x), from));
    if constexpr (sizeof(C) == 8) n += stat_from_lane(n, from);
    else n += (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)n);
  }
}

// STATS (decompress only): every lane also squares and classifies the
// elements it writes (StatAcc), each wave adds its 64 lanes up and one lane
// stores the wave's partial — no LDS, no barrier, no atomics.  A template
// parameter: under kPlanPlain the argument is S::Plan itself and the
// accumulator is StatNone, which is no code.  MEASURE is STATS without the
// stores to the wide side: the same lanes classify the same values, so the
// partials, and with them a plan's rows, are STATS's bit for bit.  SCALED
// reads its multiplier once, a wave-uniform (scalar) load beside the record's,
// and the tiles multiply every element on its way out (W::scale).
template <class S, class W, bool COMPRESS, int U, int POL, int MODE = kPlanPlain>
__global__ __launch_bounds__(kBlock) void cast_plan_kernel(typename PlanMode<S, MODE>::Arg arg) {
  constexpr bool VARIANT = MODE != kPlanPlain;
  constexpr bool STATS = MODE == kPlanStats || MODE == kPlanMeasure;
  static_assert(!(VARIANT && COMPRESS), "the variants are the decompress's");
  const typename S::Plan& p = plan_of(arg);
  // (the plain variant makes the calls below without it, as before: even an
  // empty accumulator passed by reference changed the compiler's choices in
  // the error-feedback and stochastic compresses: a 32-bit for a 64-bit compare)
  [[maybe_unused]] typename PlanMode<S, MODE>::Acc acc;
  if constexpr (MODE == kPlanScaled) acc.m = *arg.mult;
  // grid == nrecords (launch_plan_s): no bounds test in front of the record
  // load, nor of the scheme's load from its parallel array (S::state), which
  // would put a second scalar round trip before them
  const CastRec& r = p.table[blockIdx.x];
  unsigned char* const wide = r.wide;
  unsigned char* const half = r.half;
  const typename S::State st = S::state(p, blockIdx.x);  // at the record's first element
  const uint32_t kind = r.kind, count = r.count, aligned = r.aligned;
  asm volatile("" ::"s"(wide), "s"(half), "s"(kind), "s"(count), "s"(aligned));
  S::pin(p, st);
  // The record fetch is a dependent round trip at the head of every workgroup.
  // As in batched_kernel (prefetch_record), one lane touches the record of the
  // workgroup dispatched kPrefetchAhead later — the same XCD, about one
  // resident round ahead — so that it is in the XCD's L2 by then; the value is
  // consumed after the tile's own loads and stores were issued.  Two lanes,
  // the record's first and last dword, and a third for the scheme's parallel
  // entry where it has one: a lane-dependent address keeps this a vector load
  // (a uniform one becomes a scalar load with a wait right here).
  uint32_t pf = 0;
  if (threadIdx.x < 2 + S::kPlanSide && blockIdx.x + kPrefetchAhead < p.nrecords) {
    const uint32_t* rec = reinterpret_cast<const uint32_t*>(p.table + blockIdx.x + kPrefetchAhead);
    if constexpr (S::kPlanSide)
      pf = *(threadIdx.x < 2 ? rec + threadIdx.x * 7
                             : reinterpret_cast<const uint32_t*>(S::plan_side(p) + blockIdx.x +
                                                                 kPrefetchAhead));
    else
      pf = rec[threadIdx.x * 7];
  }
  const unsigned char* src = COMPRESS ? wide : half;
  unsigned char* dst = COMPRESS ? half : wide;
  const int divisor = S::divisor(p);
  const bool div = !COMPRESS && divisor > 1;
  const float fd = (float)divisor;
  if (kind == kTileFull) {
    if constexpr (VARIANT)
      cast_tile_full<S, W, COMPRESS, U, POL>(src, dst, st, div, fd, threadIdx.x, acc);
    else
      cast_tile_full<S, W, COMPRESS, U, POL>(src, dst, st, div, fd, threadIdx.x);
  } else if (kind == kTilePartial) {
    if constexpr (VARIANT)
      cast_tile_guarded<S, W, COMPRESS, U>(src, dst, st, 0, count, div, fd, threadIdx.x, acc);
    else
      cast_tile_guarded<S, W, COMPRESS, U>(src, dst, st, 0, count, div, fd, threadIdx.x);
  } else {
    CastArgs a;
    a.src = src;
    a.dst = dst;
    a.n_elems = count;  // the range [0, count) as a tail that begins at 0
    a.head = a.nunits = a.tail_begin = 0;
    a.grid = 1;
    a.divisor = divisor;
    a.aligned = (int)aligned;
    if constexpr (VARIANT)
      cast_elements<S, W, COMPRESS>(a, st, div, fd, threadIdx.x, kBlock, acc);
    else
      cast_elements<S, W, COMPRESS>(a, st, div, fd, threadIdx.x, kBlock);
  }
  if constexpr (STATS) {
    // every lane is back here, whatever it wrote (a lane that wrote nothing
    // adds 0 and 0): the record's kBlock / 64 partials are always written
    stat_wave_sum(acc.sumsq, acc.nonfinite);
    if ((threadIdx.x & 63) == 0)
      arg.part[(uint64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)] =
          StatPart{acc.sumsq, (uint64_t)acc.nonfinite};
  }
  keep_prefetch(pf);
}

// `u`: the tile size the table was cut for; `out_bytes`: what the whole launch
// writes (store policy).
template <class S, class W, bool COMPRESS>
static hipError_t launch_plan_s(const typename S::Plan& p, int u, uint64_t out_bytes,
                                const Tuning& tu, hipStream_t s) {
  if (u != 1 && u != 2 && u != 4) return hipErrorInvalidValue;
  return cast_dispatch(u, cast_store_pol(tu, out_bytes), [&](auto U, auto POL) {
    return launch_cast_kernel<cast_plan_kernel<S, W, COMPRESS, decltype(U)::value,
                                               decltype(POL)::value>>(
        p, p.nrecords, tu.occ_min_tiles_batch, tu, s);
  });
}

// The plain plan, both directions.  WIDE16: the 2-byte wide dtype of this wire
// format (the other 2-byte float).
template <class N, int WIDE16>
static hipError_t launch_plan(bool compress, const CastRec* table, uint32_t nrecords,
                              int wide_dtype, int divisor, int u, uint64_t out_bytes,
                              const Tuning& tu, hipStream_t s) {
  using S = CastPlain<N>;
  const typename S::Plan p{table, nrecords, divisor};
  switch (wide_dtype) {
    case kFloat32:
      return compress ? launch_plan_s<S, Wide<kFloat32>, true>(p, u, out_bytes, tu, s)
                      : launch_plan_s<S, Wide<kFloat32>, false>(p, u, out_bytes, tu, s);
    case kFloat64:
      return compress ? launch_plan_s<S, Wide<kFloat64>, true>(p, u, out_bytes, tu, s)
                      : launch_plan_s<S, Wide<kFloat64>, false>(p, u, out_bytes, tu, s);
    case WIDE16:
      return compress ? launch_plan_s<S, Wide<WIDE16>, true>(p, u, out_bytes, tu, s)
                      : launch_plan_s<S, Wide<WIDE16>, false>(p, u, out_bytes, tu, s);
    default: return hipErrorInvalidValue;
  }
}

// A variant of the plain plan's decompress under store policy `pol`; `p`: its
// kernel argument.
template <class N, int WIDE16, int MODE>
static hipError_t launch_plan_variant(const typename PlanMode<CastPlain<N>, MODE>::Arg& p,
                                      int wide_dtype, int u, int pol, const Tuning& tu,
                                      hipStream_t s) {
  using S = CastPlain<N>;
  if (u != 1 && u != 2 && u != 4) return hipErrorInvalidValue;
  auto go = [&](auto w) {
    using W = decltype(w);
    auto launch = [&](auto U, auto POL) {
      return launch_cast_kernel<
          cast_plan_kernel<S, W, false, decltype(U)::value, decltype(POL)::value, MODE>>(
          p, p.plan.nrecords, tu.occ_min_tiles_batch, tu, s);
    };
    if constexpr (MODE == kPlanMeasure) {  // no stores: the nt instantiation alone
      const std::integral_constant<int, kPolNt> nt;
      switch (u) {
        case 1: return launch(std::integral_constant<int, 1>{}, nt);
        case 2: return launch(std::integral_constant<int, 2>{}, nt);
        default: return launch(std::integral_constant<int, 4>{}, nt);
      }
    } else {
      return cast_dispatch(u, pol, launch);
    }
  };
  switch (wide_dtype) {
    case kFloat32: return go(Wide<kFloat32>{});
    case kFloat64: return go(Wide<kFloat64>{});
    case WIDE16: return go(Wide<WIDE16>{});
    default: return hipErrorInvalidValue;
  }
}

// The plain plan's decompress with statistics: the STATS variant, partials to
// `part` (kBlock / 64 per record).
template <class N, int WIDE16>
static hipError_t launch_plan_stats(const CastRec* table, uint32_t nrecords, int wide_dtype,
                                    int divisor, int u, uint64_t out_bytes, StatPart* part,
                                    const Tuning& tu, hipStream_t s) {
  return launch_plan_variant<N, WIDE16, kPlanStats>({{table, nrecords, divisor}, part},
                                                    wide_dtype, u, cast_store_pol(tu, out_bytes),
                                                    tu, s);
}

// The statistics alone: the MEASURE variant.  Nothing is stored to the wide
// side, so the store policy has no meaning: one instantiation.
template <class N, int WIDE16>
static hipError_t launch_plan_measure(const CastRec* table, uint32_t nrecords, int wide_dtype,
                                      int divisor, int u, StatPart* part, const Tuning& tu,
                                      hipStream_t s) {
  return launch_plan_variant<N, WIDE16, kPlanMeasure>({{table, nrecords, divisor}, part},
                                                      wide_dtype, u, kPolNt, tu, s);
}

// The decompress times `*mult` (device memory): the SCALED variant.
template <class N, int WIDE16>
static hipError_t launch_plan_scaled(const CastRec* table, uint32_t nrecords, int wide_dtype,
                                     int divisor, int u, uint64_t out_bytes, const float* mult,
                                     const Tuning& tu, hipStream_t s) {
  return launch_plan_variant<N, WIDE16, kPlanScaled>({{table, nrecords, divisor}, mult},
                                                     wide_dtype, u, cast_store_pol(tu, out_bytes),
                                                     tu, s);
}

}  // namespace bpsr
