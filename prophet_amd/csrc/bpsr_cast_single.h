// The one-tensor cast: its kernel, the cut and the launch, over the per-tile
// code of bpsr_cast_impl.h.  A template on the narrow (wire) format N, so that
// each wire format instantiates it in a translation unit of its own
// (bpsr_k_cast.hip: fp16, bpsr_k_cast_bf16.hip: bf16).  The shape is described
// in bpsr_k_cast.hip.
#pragma once

#include <cstring>

#include "bpsr_cast_impl.h"

namespace bpsr {

template <class W, class N, bool COMPRESS, int U, int POL>
__global__ __launch_bounds__(kBlock) void cast_kernel(CastArgs a) {
  asm volatile("" ::"s"(a.src), "s"(a.dst), "s"(a.nunits), "s"(a.head), "s"(a.grid),
               "s"(a.divisor));
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
  if (tile < full)
    cast_tile_full<W, N, COMPRESS, U, POL>(vsrc + tile * kTileUnits * kSrcUnit,
                                           vdst + tile * kTileUnits * kDstUnit, div, fd,
                                           threadIdx.x);
  else if (tile * kTileUnits < a.nunits)
    cast_tile_guarded<W, N, COMPRESS, U>(vsrc, vdst, tile * kTileUnits, a.nunits, div, fd,
                                         threadIdx.x);
  if (elem_mode == 2)
    cast_elements<W, N, COMPRESS>(a, div, fd, (uint64_t)blockIdx.x * kBlock + threadIdx.x,
                                  a.grid * kBlock);
  else if (elem_mode == 1)
    cast_elements<W, N, COMPRESS>(a, div, fd, threadIdx.x, kBlock);
}

template <class W, class N, bool COMPRESS, int U, int POL>
static hipError_t launch_cast_inst(const CastArgs& a, const Tuning& tu, hipStream_t s) {
  static KernelAttr attr;
  const hipError_t lds_ok =
      allow_lds(attr, reinterpret_cast<const void*>(&cast_kernel<W, N, COMPRESS, U, POL>));
  if (lds_ok != hipSuccess) return lds_ok;
  const int occ = a.grid >= tu.occ_min_tiles ? tu.copy_occ : 0;
  hipLaunchKernelGGL((cast_kernel<W, N, COMPRESS, U, POL>), dim3((uint32_t)a.grid),
                     dim3(kBlock), occ_lds_bytes(occ), s, a);
  return hipGetLastError();
}

template <class W, class N, bool COMPRESS>
static hipError_t launch_cast_dir(const CastArgs& a, int u, int pol, const Tuning& tu,
                                  hipStream_t s) {
  if (pol == kPolWt) {
    switch (u) {
      case 1: return launch_cast_inst<W, N, COMPRESS, 1, kPolWt>(a, tu, s);
      case 2: return launch_cast_inst<W, N, COMPRESS, 2, kPolWt>(a, tu, s);
      default: return launch_cast_inst<W, N, COMPRESS, 4, kPolWt>(a, tu, s);
    }
  }
  switch (u) {
    case 1: return launch_cast_inst<W, N, COMPRESS, 1, kPolNt>(a, tu, s);
    case 2: return launch_cast_inst<W, N, COMPRESS, 2, kPolNt>(a, tu, s);
    default: return launch_cast_inst<W, N, COMPRESS, 4, kPolNt>(a, tu, s);
  }
}

// Geometry of one cast: h = the narrow operand, w = the wide one (es bytes per
// element), cut by cast_cut (bpsr_internal.h; the cast plan's table builder
// cuts its segments with the same function).
static void cast_geom(const void* h, const void* w, size_t nelem, int es, CastArgs* a) {
  const CastCut c = cast_cut(h, w, nelem, es);
  a->n_elems = nelem;
  a->aligned = c.aligned;
  a->head = c.head;
  a->nunits = c.nunits;
  a->tail_begin = c.nunits ? c.head + c.nunits * 8 : 0;
}

// WIDE16: the 2-byte wide dtype of this wire format (the other 2-byte float).
template <class N, int WIDE16>
static hipError_t launch_cast(bool compress, void* dst, const void* src, size_t nelem, int dtype,
                              int divisor, const Tuning& tu, hipStream_t s) {
  const int es = elem_size(dtype);
  CastArgs a;
  std::memset(&a, 0, sizeof(a));
  a.src = static_cast<const unsigned char*>(src);
  a.dst = static_cast<unsigned char*>(dst);
  a.divisor = divisor;
  cast_geom(compress ? dst : src, compress ? src : dst, nelem, es, &a);
  auto tiles = [&a](int u) { return (a.nunits + (uint64_t)kBlock * u - 1) / ((uint64_t)kBlock * u); };
  int u = tu.copy_vpt;
  while (u > 1 && tiles(u) < kMinTiles) u >>= 1;
  uint64_t grid = tiles(u);
  if (grid == 0) {
    grid = (nelem + kBlock - 1) / kBlock;
    if (grid > 65536) grid = 65536;
  }
  if (grid > 0x7fffffffull) return hipErrorInvalidValue;
  a.grid = grid;
  Tuning tn = tu;
  tn.nt = 1;  // streaming: every byte is read once
  const int pol = cache_pol(tn, (uint64_t)nelem * (compress ? 2 : (uint64_t)es));
  switch (dtype) {
    case kFloat32:
      return compress ? launch_cast_dir<Wide<kFloat32>, N, true>(a, u, pol, tu, s)
                      : launch_cast_dir<Wide<kFloat32>, N, false>(a, u, pol, tu, s);
    case kFloat64:
      return compress ? launch_cast_dir<Wide<kFloat64>, N, true>(a, u, pol, tu, s)
                      : launch_cast_dir<Wide<kFloat64>, N, false>(a, u, pol, tu, s);
    case WIDE16:
      return compress ? launch_cast_dir<Wide<WIDE16>, N, true>(a, u, pol, tu, s)
                      : launch_cast_dir<Wide<WIDE16>, N, false>(a, u, pol, tu, s);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace bpsr
