// The cast plan's kernel and launch over the per-tile code of
// bpsr_cast_impl.h.  A template on the rounding scheme S and with it the narrow
// (wire) format, so that each (scheme, wire format) instantiates it in a
// translation unit of its own (plain: bpsr_k_cast_plan.hip,
// bpsr_k_cast_plan_bf16.hip; error feedback: bpsr_k_cast_ef*.hip; stochastic
// rounding: bpsr_k_cast_sr*.hip).  What a plan is and how a record is read:
// bpsr_k_cast_plan.hip.
#pragma once

#include "bpsr_cast_impl.h"

namespace bpsr {

template <class S, class W, bool COMPRESS, int U, int POL>
__global__ __launch_bounds__(kBlock) void cast_plan_kernel(typename S::Plan p) {
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
    cast_tile_full<S, W, COMPRESS, U, POL>(src, dst, st, div, fd, threadIdx.x);
  } else if (kind == kTilePartial) {
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
    cast_elements<S, W, COMPRESS>(a, st, div, fd, threadIdx.x, kBlock);
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

}  // namespace bpsr
