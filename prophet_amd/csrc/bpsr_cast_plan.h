// The cast plan's kernel and launch over the per-tile code of
// bpsr_cast_impl.h.  A template on the narrow (wire) format N, so that each
// wire format instantiates it in a translation unit of its own
// (bpsr_k_cast_plan.hip: fp16, bpsr_k_cast_plan_bf16.hip: bf16).  What a plan
// is and how a record is read: bpsr_k_cast_plan.hip.
#pragma once

#include "bpsr_cast_impl.h"

namespace bpsr {

template <class W, class N, bool COMPRESS, int U, int POL>
__global__ __launch_bounds__(kBlock) void cast_plan_kernel(const CastRec* __restrict__ table,
                                                           uint32_t nrecords, int divisor) {
  // grid == nrecords (launch_plan_inst): no bounds test in front of the record
  // load, which would put a second scalar round trip before it
  const CastRec& r = table[blockIdx.x];
  unsigned char* const wide = r.wide;
  unsigned char* const half = r.half;
  const uint32_t kind = r.kind, count = r.count, aligned = r.aligned;
  asm volatile("" ::"s"(wide), "s"(half), "s"(kind), "s"(count), "s"(aligned), "s"(divisor));
  // The record fetch is a dependent round trip at the head of every workgroup.
  // As in batched_kernel (prefetch_record), one lane touches the record of the
  // workgroup dispatched kPrefetchAhead later — the same XCD, about one
  // resident round ahead — so that it is in the XCD's L2 by then; the value is
  // consumed after the tile's own loads and stores were issued.  Two lanes,
  // the record's first and last dword: a lane-dependent address keeps this a
  // vector load (a uniform one becomes a scalar load with a wait right here).
  uint32_t pf = 0;
  if (threadIdx.x < 2 && blockIdx.x + kPrefetchAhead < nrecords)
    pf = reinterpret_cast<const uint32_t*>(table + blockIdx.x + kPrefetchAhead)[threadIdx.x * 7];
  const unsigned char* src = COMPRESS ? wide : half;
  unsigned char* dst = COMPRESS ? half : wide;
  const bool div = !COMPRESS && divisor > 1;
  const float fd = (float)divisor;
  if (kind == kTileFull) {
    cast_tile_full<W, N, COMPRESS, U, POL>(src, dst, div, fd, threadIdx.x);
  } else if (kind == kTilePartial) {
    cast_tile_guarded<W, N, COMPRESS, U>(src, dst, 0, count, div, fd, threadIdx.x);
  } else {
    CastArgs a;
    a.src = src;
    a.dst = dst;
    a.n_elems = count;  // the range [0, count) as a tail that begins at 0
    a.head = a.nunits = a.tail_begin = 0;
    a.grid = 1;
    a.divisor = divisor;
    a.aligned = (int)aligned;
    cast_elements<W, N, COMPRESS>(a, div, fd, threadIdx.x, kBlock);
  }
  keep_prefetch(pf);
}

template <class W, class N, bool COMPRESS, int U, int POL>
static hipError_t launch_plan_inst(const CastRec* table, uint32_t nrecords, int divisor,
                                   const Tuning& tu, hipStream_t s) {
  static KernelAttr attr;
  const hipError_t lds_ok = allow_lds(
      attr, reinterpret_cast<const void*>(&cast_plan_kernel<W, N, COMPRESS, U, POL>));
  if (lds_ok != hipSuccess) return lds_ok;
  const int occ = nrecords >= tu.occ_min_tiles_batch ? tu.copy_occ : 0;
  hipLaunchKernelGGL((cast_plan_kernel<W, N, COMPRESS, U, POL>), dim3(nrecords), dim3(kBlock),
                     occ_lds_bytes(occ), s, table, nrecords, divisor);
  return hipGetLastError();
}

template <class W, class N, bool COMPRESS>
static hipError_t launch_plan_dir(const CastRec* table, uint32_t nrecords, int divisor, int u,
                                  int pol, const Tuning& tu, hipStream_t s) {
  if (pol == kPolWt) {
    switch (u) {
      case 1: return launch_plan_inst<W, N, COMPRESS, 1, kPolWt>(table, nrecords, divisor, tu, s);
      case 2: return launch_plan_inst<W, N, COMPRESS, 2, kPolWt>(table, nrecords, divisor, tu, s);
      default: return launch_plan_inst<W, N, COMPRESS, 4, kPolWt>(table, nrecords, divisor, tu, s);
    }
  }
  switch (u) {
    case 1: return launch_plan_inst<W, N, COMPRESS, 1, kPolNt>(table, nrecords, divisor, tu, s);
    case 2: return launch_plan_inst<W, N, COMPRESS, 2, kPolNt>(table, nrecords, divisor, tu, s);
    default: return launch_plan_inst<W, N, COMPRESS, 4, kPolNt>(table, nrecords, divisor, tu, s);
  }
}

// WIDE16: the 2-byte wide dtype of this wire format (the other 2-byte float).
template <class N, int WIDE16>
static hipError_t launch_plan(bool compress, const CastRec* table, uint32_t nrecords,
                              int wide_dtype, int divisor, int u, uint64_t out_bytes,
                              const Tuning& tu, hipStream_t s) {
  if (u != 1 && u != 2 && u != 4) return hipErrorInvalidValue;
  Tuning tn = tu;
  tn.nt = 1;  // streaming: every byte is read once
  const int pol = cache_pol(tn, out_bytes);
  switch (wide_dtype) {
    case kFloat32:
      return compress ? launch_plan_dir<Wide<kFloat32>, N, true>(table, nrecords, divisor, u, pol,
                                                                 tu, s)
                      : launch_plan_dir<Wide<kFloat32>, N, false>(table, nrecords, divisor, u, pol,
                                                                  tu, s);
    case kFloat64:
      return compress ? launch_plan_dir<Wide<kFloat64>, N, true>(table, nrecords, divisor, u, pol,
                                                                 tu, s)
                      : launch_plan_dir<Wide<kFloat64>, N, false>(table, nrecords, divisor, u, pol,
                                                                  tu, s);
    case WIDE16:
      return compress ? launch_plan_dir<Wide<WIDE16>, N, true>(table, nrecords, divisor, u, pol,
                                                               tu, s)
                      : launch_plan_dir<Wide<WIDE16>, N, false>(table, nrecords, divisor, u, pol,
                                                                tu, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace bpsr
