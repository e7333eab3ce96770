// The one-tensor cast: its kernel, the launch rule and the launch, over the
// per-tile code of bpsr_cast_impl.h.  A template on the rounding scheme S and
// with it the narrow (wire) format, so that each (scheme, wire format)
// instantiates it in a translation unit of its own (plain: bpsr_k_cast.hip,
// bpsr_k_cast_bf16.hip; error feedback: bpsr_k_cast_ef*.hip; stochastic
// rounding: bpsr_k_cast_sr*.hip).  The shape is described in bpsr_k_cast.hip.
#pragma once

#include <cstring>

#include "bpsr_cast_impl.h"

namespace bpsr {

template <class S, class W, bool COMPRESS, int U, int POL>
__global__ __launch_bounds__(kBlock) void cast_kernel(typename S::Single p) {
  const CastArgs& a = p.a;
  const typename S::State st = S::state(p);  // at element 0
  asm volatile("" ::"s"(a.src), "s"(a.dst), "s"(a.nunits), "s"(a.head), "s"(a.grid));
  S::pin(p, st);
  constexpr uint64_t kTileUnits = (uint64_t)kBlock * U;
  constexpr uint64_t kSrcUnit = COMPRESS ? 16 * W::kVecs : 16;  // bytes per unit
  constexpr uint64_t kDstUnit = COMPRESS ? 16 : 16 * W::kVecs;
  constexpr uint64_t kSrcElem = COMPRESS ? sizeof(typename W::E) : 2;
  constexpr uint64_t kDstElem = COMPRESS ? 2 : sizeof(typename W::E);
  const bool div = !COMPRESS && a.divisor > 1;
  const float fd = (float)a.divisor;
  const uint64_t full = a.nunits / kTileUnits;
  const bool partial = full * kTileUnits < a.nunits;
  const uint64_t bid = blockIdx.x;
  const int elem_mode = a.nunits == 0 ? 2 : (bid == 0 ? 1 : 0);
  // workgroup 0 takes the partial tile (if any) and the element work, the full
  // tiles follow in address order (fold_kernel's dispatch order)
  const uint64_t tile = partial ? (bid == 0 ? full : bid - 1) : bid;
  const unsigned char* vsrc = a.src + a.head * kSrcElem;
  unsigned char* vdst = a.dst + a.head * kDstElem;
  const typename S::State vst = st.at(a.head);  // at the vector range
  if (tile < full)
    cast_tile_full<S, W, COMPRESS, U, POL>(vsrc + tile * kTileUnits * kSrcUnit,
                                           vdst + tile * kTileUnits * kDstUnit,
                                           vst.at(tile * kTileUnits * 8), div, fd, threadIdx.x);
  else if (tile * kTileUnits < a.nunits)
    cast_tile_guarded<S, W, COMPRESS, U>(vsrc, vdst, vst, tile * kTileUnits, a.nunits, div, fd,
                                         threadIdx.x);
  if (elem_mode == 2)
    cast_elements<S, W, COMPRESS>(a, st, div, fd, (uint64_t)blockIdx.x * kBlock + threadIdx.x,
                                  a.grid * kBlock);
  else if (elem_mode == 1)
    cast_elements<S, W, COMPRESS>(a, st, div, fd, threadIdx.x, kBlock);
}

// The launch rule of every one-tensor cast: the cut `c` (cast_cut or
// cast_cut_ef, bpsr_internal.h; the cast plan's table builder cuts its
// segments with the same functions) as CastArgs, the tile size *u = copy_vpt,
// halved while there would be fewer than kMinTiles tiles, and one workgroup
// per tile — or, without a vector range, per kBlock elements.
static hipError_t cast_rule(const CastCut& c, void* dst, const void* src, size_t nelem,
                            int divisor, const Tuning& tu, CastArgs* a, int* u) {
  std::memset(a, 0, sizeof(*a));
  a->src = static_cast<const unsigned char*>(src);
  a->dst = static_cast<unsigned char*>(dst);
  a->divisor = divisor;
  a->n_elems = nelem;
  a->aligned = c.aligned;
  a->head = c.head;
  a->nunits = c.nunits;
  a->tail_begin = c.nunits ? c.head + c.nunits * 8 : 0;
  auto tiles = [a](uint64_t v) { return (a->nunits + kBlock * v - 1) / (kBlock * v); };
  *u = tu.copy_vpt;
  while (*u > 1 && tiles(*u) < kMinTiles) *u >>= 1;
  uint64_t grid = tiles(*u);
  if (grid == 0) {
    grid = (nelem + kBlock - 1) / kBlock;
    if (grid > 65536) grid = 65536;
  }
  if (grid > 0x7fffffffull) return hipErrorInvalidValue;
  a->grid = grid;
  return hipSuccess;
}

// p.a from cast_rule; `out_bytes`: what the launch writes (store policy).
template <class S, class W, bool COMPRESS>
static hipError_t launch_single(const typename S::Single& p, int u, uint64_t out_bytes,
                                const Tuning& tu, hipStream_t s) {
  return cast_dispatch(u, cast_store_pol(tu, out_bytes), [&](auto U, auto POL) {
    return launch_cast_kernel<cast_kernel<S, W, COMPRESS, decltype(U)::value,
                                          decltype(POL)::value>>(p, p.a.grid, tu.occ_min_tiles,
                                                                 tu, s);
  });
}

// The plain cast, both directions.  WIDE16: the 2-byte wide dtype of this wire
// format (the other 2-byte float).
template <class N, int WIDE16>
static hipError_t launch_cast(bool compress, void* dst, const void* src, size_t nelem, int dtype,
                              int divisor, const Tuning& tu, hipStream_t s) {
  using S = CastPlain<N>;
  const int es = elem_size(dtype);
  typename S::Single p;
  int u;
  const hipError_t e = cast_rule(cast_cut(compress ? dst : src, compress ? src : dst, nelem, es),
                                 dst, src, nelem, divisor, tu, &p.a, &u);
  if (e != hipSuccess) return e;
  const uint64_t out = (uint64_t)nelem * (compress ? 2 : (uint64_t)es);
  switch (dtype) {
    case kFloat32:
      return compress ? launch_single<S, Wide<kFloat32>, true>(p, u, out, tu, s)
                      : launch_single<S, Wide<kFloat32>, false>(p, u, out, tu, s);
    case kFloat64:
      return compress ? launch_single<S, Wide<kFloat64>, true>(p, u, out, tu, s)
                      : launch_single<S, Wide<kFloat64>, false>(p, u, out, tu, s);
    case WIDE16:
      return compress ? launch_single<S, Wide<WIDE16>, true>(p, u, out, tu, s)
                      : launch_single<S, Wide<WIDE16>, false>(p, u, out, tu, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace bpsr
