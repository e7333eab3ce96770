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

#include "bpsr_kernels_impl.h"

namespace bpsr {

// Wide-side element: its 16-B vectors per unit, and the exact steps to and
// from f32 bits.  get/put address element e (0..7) of a unit's vectors.
template <int DT>
struct Wide;

template <>
struct Wide<kFloat32> {
  using E = uint32_t;
  static constexpr int kVecs = 2;
  __device__ static uint32_t to_f32(E x) { return x; }
  __device__ static E from_f32(float f) { return bitcast<uint32_t>(f); }
  __device__ static E get(const vec16* x, int e) { return x[e >> 2].w[e & 3]; }
  __device__ static void put(vec16* x, int e, E v) { x[e >> 2].w[e & 3] = v; }
};

template <>
struct Wide<kFloat64> {
  using E = uint64_t;
  static constexpr int kVecs = 4;
  // round to f32 first (RNE), as the host conversion does
  __device__ static uint32_t to_f32(E x) { return bitcast<uint32_t>((float)bitcast<double>(x)); }
  __device__ static E from_f32(float f) { return bitcast<uint64_t>((double)f); }
  __device__ static E get(const vec16* x, int e) {
    return ((uint64_t)x[e >> 1].w[(e & 1) * 2 + 1] << 32) | x[e >> 1].w[(e & 1) * 2];
  }
  __device__ static void put(vec16* x, int e, E v) {
    x[e >> 1].w[(e & 1) * 2] = (uint32_t)v;
    x[e >> 1].w[(e & 1) * 2 + 1] = (uint32_t)(v >> 32);
  }
};

template <>
struct Wide<kBFloat16> {
  using E = uint16_t;
  static constexpr int kVecs = 1;
  __device__ static uint32_t to_f32(E x) { return (uint32_t)x << 16; }  // exact
  __device__ static E from_f32(float f) { return (E)f32_to_bf16_rne(bitcast<uint32_t>(f)); }
  __device__ static E get(const vec16* x, int e) {
    return (E)(x[0].w[e >> 1] >> ((e & 1) * 16));
  }
  __device__ static void put(vec16* x, int e, E v) {
    if (e & 1) x[0].w[e >> 1] |= (uint32_t)v << 16;
    else x[0].w[e >> 1] = v;
  }
};

struct CastArgs {
  const unsigned char* src;
  unsigned char* dst;
  uint64_t n_elems;
  uint64_t head;        // elements before the vector range
  uint64_t nunits;      // 8-element units in the vector range
  uint64_t tail_begin;  // head + 8 * nunits
  uint64_t grid;        // launched workgroups
  int divisor;          // decompress: >= 1
  int aligned;          // both operands element-aligned
};

template <class W>
__device__ __forceinline__ uint16_t compress_elem(typename W::E x) {
  return (uint16_t)f2h_bits(W::to_f32(x));
}

// div: the quotient is rounded to fp16 BEFORE it is widened.
template <class W>
__device__ __forceinline__ typename W::E decompress_elem(uint16_t h, bool div, float fd) {
  if (div) h = (uint16_t)f2h_bits(bitcast<uint32_t>((float)bitcast<_Float16>(h) / fd));
  return W::from_f32((float)bitcast<_Float16>(h));
}

template <class W>
__device__ __forceinline__ vec16 compress_unit(const vec16* x) {
  vec16 o;
#pragma unroll
  for (int e = 0; e < 8; e += 2)
    o.w[e >> 1] = (uint32_t)compress_elem<W>(W::get(x, e)) |
                  ((uint32_t)compress_elem<W>(W::get(x, e + 1)) << 16);
  return o;
}

template <class W>
__device__ __forceinline__ void decompress_unit(const vec16& h, bool div, float fd, vec16* o) {
#pragma unroll
  for (int e = 0; e < 8; ++e)
    W::put(o, e, decompress_elem<W>((uint16_t)(h.w[e >> 1] >> ((e & 1) * 16)), div, fd));
}

// Full tile: units [0, kBlock * U) of the tile whose first bytes are h0 (fp16
// side) and w0 (wide side); lane handles units lane + j * kBlock.  One buffer
// descriptor per operand sized to the tile, 32-bit lane offsets.
template <class W, bool COMPRESS, int U, int POL>
__device__ __forceinline__ void cast_tile_full(const unsigned char* src, unsigned char* dst,
                                               bool div, float fd, int lane) {
  constexpr int kAux = 2;                            // loads: nt
  constexpr int kStAux = POL == kPolWt ? 16 : kAux;  // stores: sc1 (write-through) or nt
  constexpr int KV = W::kVecs;
  constexpr int kHBytes = kBlock * U * 16, kWBytes = kHBytes * KV;
  typedef uint32_t u4 __attribute__((ext_vector_type(4)));
  const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(src), 0,
                                                    COMPRESS ? kWBytes : kHBytes, 0x00020000);
  const auto rd = __builtin_amdgcn_make_buffer_rsrc(dst, 0, COMPRESS ? kHBytes : kWBytes,
                                                    0x00020000);
  if constexpr (COMPRESS && KV > 1) {
    // The mirror image of the decompress below: load instruction v reads the
    // wave's input vectors v * 64 + l (1 KiB contiguous), each lane rounds the
    // elements it loaded, and lane l collects the fp16 values of ITS unit
    // (vectors l * KV + s, all in load l / (64 / KV)) from the lanes that
    // hold them.  Every element is rounded exactly once, by the lane that
    // loaded it.
    constexpr int EPV = 8 / KV, DW = EPV / 2;  // elements / fp16 dwords per input vector
    const int l = lane & 63, wave0 = lane & ~63;
    vec16 x[U][KV];
#pragma unroll
    for (int j = 0; j < U; ++j)
#pragma unroll
      for (int v = 0; v < KV; ++v)
        x[j][v] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(
            rs, ((j * kBlock + wave0) * KV + v * 64 + l) * 16, 0, kAux));
    const int vi = l / (64 / KV);
#pragma unroll
    for (int j = 0; j < U; ++j) {
      uint32_t c[KV][DW];
#pragma unroll
      for (int v = 0; v < KV; ++v)
#pragma unroll
        for (int k = 0; k < DW; ++k)
          c[v][k] = (uint32_t)compress_elem<W>(W::get(&x[j][v], 2 * k)) |
                    ((uint32_t)compress_elem<W>(W::get(&x[j][v], 2 * k + 1)) << 16);
      vec16 o;
#pragma unroll
      for (int s = 0; s < KV; ++s) {
        const int from = ((l * KV + s) & 63) * 4;
#pragma unroll
        for (int k = 0; k < DW; ++k) {
          uint32_t r = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)c[0][k]);
#pragma unroll
          for (int v = 1; v < KV; ++v) {
            const uint32_t t = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)c[v][k]);
            r = vi == v ? t : r;
          }
          o.w[s * DW + k] = r;
        }
      }
      __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(o), rd, (j * kBlock + lane) * 16, 0,
                                             kStAux);
    }
  } else if constexpr (COMPRESS) {
    vec16 x[U][KV];
#pragma unroll
    for (int j = 0; j < U; ++j)
#pragma unroll
      for (int v = 0; v < KV; ++v)
        x[j][v] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(
            rs, ((j * kBlock + lane) * KV + v) * 16, 0, kAux));
#pragma unroll
    for (int j = 0; j < U; ++j)
      __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(compress_unit<W>(x[j])), rd,
                                             (j * kBlock + lane) * 16, 0, kStAux);
  } else {
    vec16 h[U];
#pragma unroll
    for (int j = 0; j < U; ++j)
      h[j] = bitcast<vec16>(
          __builtin_amdgcn_raw_buffer_load_b128(rs, (j * kBlock + lane) * 16, 0, kAux));
    if constexpr (KV > 1) {
      // Lane-private stores would leave each store instruction writing 16 of
      // every 16 * KV bytes — a fraction of each 128-B line per instruction,
      // measured 0.53 (no divide) to 0.59 of the roofline for f32, so it was
      // the store pattern and not the divide that bound it; re-dealt, 0.75
      // with or without the divide.  So the wave's 64 units are
      // re-dealt before the widen: store instruction v writes the wave's
      // output vectors v * 64 + l, 1 KiB contiguous, and lane l fetches the
      // fp16 values of that vector from the lane that loaded them (unit
      // (v * 64 + l) / KV, its sub-vector (v * 64 + l) % KV) by ds_bpermute —
      // the halves travel, 2 bytes an element, and each element is still
      // divided and widened exactly once.  Full tiles only: every lane is
      // active.
      constexpr int EPV = 8 / KV;  // elements per output vector
      const int l = lane & 63, wave0 = lane & ~63;
#pragma unroll
      for (int j = 0; j < U; ++j) {
#pragma unroll
        for (int v = 0; v < KV; ++v) {
          const int g = v * 64 + l;
          const int from = (g / KV) * 4, sub = g % KV;
          uint32_t w[4];
#pragma unroll
          for (int k = 0; k < 4; ++k)
            w[k] = (uint32_t)__builtin_amdgcn_ds_bpermute(from, (int)h[j].w[k]);
          // the EPV halves of sub-vector `sub`: dwords [sub * EPV / 2, + EPV / 2)
          uint32_t d[EPV / 2];
#pragma unroll
          for (int k = 0; k < EPV / 2; ++k) {
            d[k] = w[k];
#pragma unroll
            for (int s = 1; s < KV; ++s) d[k] = sub == s ? w[s * (EPV / 2) + k] : d[k];
          }
          vec16 o{};
#pragma unroll
          for (int e = 0; e < EPV; ++e)  // e < EPV: all within the one vector
            W::put(&o, e, decompress_elem<W>((uint16_t)(d[e >> 1] >> ((e & 1) * 16)), div, fd));
          __builtin_amdgcn_raw_buffer_store_b128(
              bitcast<u4>(o), rd, ((j * kBlock + wave0) * KV + g) * 16, 0, kStAux);
        }
      }
      return;
    }
#pragma unroll
    for (int j = 0; j < U; ++j) {
      vec16 o[KV];
      decompress_unit<W>(h[j], div, fd, o);
#pragma unroll
      for (int v = 0; v < KV; ++v)
        __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(o[v]), rd,
                                               ((j * kBlock + lane) * KV + v) * 16, 0, kStAux);
    }
  }
}

// The partial last tile: units [u0, nunits) of the vector range (src / dst
// already advanced to the range); a unit past nunits is neither read nor
// written.
template <class W, bool COMPRESS, int U>
__device__ __forceinline__ void cast_tile_guarded(const unsigned char* src, unsigned char* dst,
                                                  uint64_t u0, uint64_t nunits, bool div,
                                                  float fd, int lane) {
  constexpr int KV = W::kVecs;
#pragma unroll
  for (int j = 0; j < U; ++j) {
    const uint64_t u = u0 + (uint64_t)j * kBlock + lane;
    if (u >= nunits) continue;
    if constexpr (COMPRESS) {
      vec16 x[KV];
#pragma unroll
      for (int v = 0; v < KV; ++v) x[v] = ld16<true>(src + (u * KV + v) * 16);
      st16<true>(dst + u * 16, compress_unit<W>(x));
    } else {
      vec16 o[KV];
      decompress_unit<W>(ld16<true>(src + u * 16), div, fd, o);
#pragma unroll
      for (int v = 0; v < KV; ++v) st16<true>(dst + (u * KV + v) * 16, o[v]);
    }
  }
}

// Elements [0, head) and [tail_begin, n_elems), one per thread.
template <class W, bool COMPRESS>
__device__ __forceinline__ void cast_elements(const CastArgs& a, bool div, float fd, uint64_t t,
                                              uint64_t stride) {
  using E = typename W::E;
  const bool al = a.aligned != 0;
  const uint64_t n_scalar = a.head + (a.n_elems - a.tail_begin);
  for (uint64_t s = t; s < n_scalar; s += stride) {
    const uint64_t e = s < a.head ? s : a.tail_begin + (s - a.head);
    if constexpr (COMPRESS)
      st_e<uint16_t>(a.dst + e * 2, compress_elem<W>(ld_e<E>(a.src + e * sizeof(E), al)), al);
    else
      st_e<E>(a.dst + e * sizeof(E), decompress_elem<W>(ld_e<uint16_t>(a.src + e * 2, al), div, fd),
              al);
  }
}

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
// element).  The vector range starts at the first element index where both
// are 16-byte aligned: the fp16 side every 8 elements from hh, the wide side
// every 16 / es from hw, so they meet iff hh = hw mod (16 / es), first at hh.
static void cast_geom(const void* h, const void* w, size_t nelem, int es, CastArgs* a) {
  const uintptr_t ph = (uintptr_t)h, pw = (uintptr_t)w;
  a->n_elems = nelem;
  a->aligned = (ph % 2 == 0 && pw % (uintptr_t)es == 0) ? 1 : 0;
  a->head = a->nunits = a->tail_begin = 0;
  if (!a->aligned) return;
  const uint64_t hh = ((16 - (ph & 15)) & 15) / 2;
  const uint64_t hw = ((16 - (pw & 15)) & 15) / (uint64_t)es;
  if (hh % (16 / (uint64_t)es) != hw || hh >= nelem) return;
  a->nunits = (nelem - hh) / 8;
  if (a->nunits == 0) return;
  a->head = hh;
  a->tail_begin = hh + a->nunits * 8;
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
