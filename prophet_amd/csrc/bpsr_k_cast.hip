// FP16 gradient compression (byteps/torch/compression.py, FP16Compressor) on
// the device: the cast to fp16 before a push and the cast back after the pull,
// the latter fused with push_pull(average=True)'s divide.
//
//   compress    f16[i] = rne_f16(float(src[i]))        src: f32, f64 or bf16
//   decompress  dst[i] = T(h[i])                        divisor 1
//               dst[i] = T(rne_f16(float(h[i]) / float(divisor)))   divisor > 1
//
// The reference divides the COMPRESSED tensor in place (torch/ops.cc:77-81:
// the callback's div_ runs on the fp16 output) and widens afterwards, so the
// quotient is rounded to fp16 before it is widened; that is what the host
// does (Half / Half: a float divide rounded back to Half), and what this
// kernel pins bit for bit.  f64 goes through f32 first (the host conversion's
// double rounding: 1 + 2^-11 + 2^-30 gives 1.0).  NaN in, NaN out (f2h_bits'
// payload rule; the payload is not part of the contract).  The divide is a
// plain IEEE `/`: no reciprocal, no fast-math (Makefile).
//
// Shape: a streaming kernel over two operands of unequal element width, cut
// like the copy (bpsr_k_copy.hip).  A lane's unit is 8 elements: ONE 16-byte
// vector on the fp16 side and kVecs (f32: 2, f64: 4, bf16: 1) 16-byte vectors
// on the wide side, so both sides move 16 bytes per access.  A tile is
// kBlock * U units (U = the copy's vectors per thread, halved while the launch
// would have fewer than kMinTiles tiles), one workgroup per tile, full tiles
// through buffer instructions (nt loads; write-through stores below
// Tuning::wt_max_bytes of output, nt above), residency Tuning::copy_occ.  In
// a full tile the wide side's instruction v of a wave touches the wave's
// vectors v * 64 + lane — 1 KiB contiguous — and the fp16 values change lanes
// by ds_bpermute (cast_tile_full): with lane-private wide vectors every
// instruction touched 16 of each 16 * kVecs bytes, and the f32 decompress ran
// at 0.53-0.59 of the roofline instead of 0.75, the compress at 0.74 instead
// of 0.78 (tools/bench_compress.py, profiles/README.md).  The
// vector range starts at the first element where BOTH operands are 16-byte
// aligned; the elements before it, the tail past the last whole unit and the
// guarded partial tile go to workgroup 0 (first off the dispatcher, as in
// fold_kernel).  Operands that never co-align go through the element path
// entirely.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#include "bpsr_cast_impl.h"

namespace bpsr {

template <class W, bool COMPRESS, int U, int POL>
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
    cast_tile_full<W, COMPRESS, U, POL>(vsrc + tile * kTileUnits * kSrcUnit,
                                        vdst + tile * kTileUnits * kDstUnit, div, fd,
                                        threadIdx.x);
  else if (tile * kTileUnits < a.nunits)
    cast_tile_guarded<W, COMPRESS, U>(vsrc, vdst, tile * kTileUnits, a.nunits, div, fd,
                                      threadIdx.x);
  if (elem_mode == 2)
    cast_elements<W, COMPRESS>(a, div, fd, (uint64_t)blockIdx.x * kBlock + threadIdx.x,
                               a.grid * kBlock);
  else if (elem_mode == 1)
    cast_elements<W, COMPRESS>(a, div, fd, threadIdx.x, kBlock);
}

template <class W, bool COMPRESS, int U, int POL>
static hipError_t launch_cast_inst(const CastArgs& a, const Tuning& tu, hipStream_t s) {
  static KernelAttr attr;
  const hipError_t lds_ok =
      allow_lds(attr, reinterpret_cast<const void*>(&cast_kernel<W, COMPRESS, U, POL>));
  if (lds_ok != hipSuccess) return lds_ok;
  const int occ = a.grid >= tu.occ_min_tiles ? tu.copy_occ : 0;
  hipLaunchKernelGGL((cast_kernel<W, COMPRESS, U, POL>), dim3((uint32_t)a.grid), dim3(kBlock),
                     occ_lds_bytes(occ), s, a);
  return hipGetLastError();
}

template <class W, bool COMPRESS>
static hipError_t launch_cast_dir(const CastArgs& a, int u, int pol, const Tuning& tu,
                                  hipStream_t s) {
  if (pol == kPolWt) {
    switch (u) {
      case 1: return launch_cast_inst<W, COMPRESS, 1, kPolWt>(a, tu, s);
      case 2: return launch_cast_inst<W, COMPRESS, 2, kPolWt>(a, tu, s);
      default: return launch_cast_inst<W, COMPRESS, 4, kPolWt>(a, tu, s);
    }
  }
  switch (u) {
    case 1: return launch_cast_inst<W, COMPRESS, 1, kPolNt>(a, tu, s);
    case 2: return launch_cast_inst<W, COMPRESS, 2, kPolNt>(a, tu, s);
    default: return launch_cast_inst<W, COMPRESS, 4, kPolNt>(a, tu, s);
  }
}

// Geometry of one cast: h = the fp16 operand, w = the wide one (es bytes per
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
      return compress ? launch_cast_dir<Wide<kFloat32>, true>(a, u, pol, tu, s)
                      : launch_cast_dir<Wide<kFloat32>, false>(a, u, pol, tu, s);
    case kFloat64:
      return compress ? launch_cast_dir<Wide<kFloat64>, true>(a, u, pol, tu, s)
                      : launch_cast_dir<Wide<kFloat64>, false>(a, u, pol, tu, s);
    case kBFloat16:
      return compress ? launch_cast_dir<Wide<kBFloat16>, true>(a, u, pol, tu, s)
                      : launch_cast_dir<Wide<kBFloat16>, false>(a, u, pol, tu, s);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_compress_fp16(void* dst, const void* src, size_t nelem, int src_dtype,
                                const Tuning& tu, hipStream_t s) {
  return launch_cast(true, dst, src, nelem, src_dtype, 1, tu, s);
}

hipError_t launch_decompress_fp16(void* dst, const void* src, size_t nelem, int dst_dtype,
                                  int divisor, const Tuning& tu, hipStream_t s) {
  return launch_cast(false, dst, src, nelem, dst_dtype, divisor, tu, s);
}

}  // namespace bpsr
