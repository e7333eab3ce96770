// The block-scaled wires over 2-byte gradients: bpsr_k_mx.hip's and
// bpsr_k_mx_sr.hip's four kernels for fp16 and bf16 tensors (DESIGN.md §11.16;
// the definitions are prophet_amd/mx.py and prophet_amd/mx_sr.py).  An element
// is widened exactly to f32 as it is loaded and everything after that is the
// f32 kernels' arithmetic, so the payload is the one its f32 upcast gives; a
// fold converts its f32 result once, as the casts do (Wide<DT>::from_f32:
// nearest even, overflow to infinity, subnormals kept, the casts' NaN bits).
// The residual of the error-feedback wire stays f32.
//
//   EF COMPRESS  c = f32(g) + r; X, codes and r' as bpsr_k_mx.hip
//   SR COMPRESS  [c = H D f32(g), whole blocks;] X and codes as bpsr_k_mx_sr.hip
//   FOLD         out = half((d_0 + ... + d_{N-1}) [/ divisor])
//   RHT FOLD     out = half(D H t 2^-5 [/ divisor])
//
// Each is one launch, one workgroup a tile record, no scratch memory.
//
// The lane map is the 8-element one.  A tile is still 4,096 elements, 8 KiB
// of the 2-byte operand: 512 units of one b128, 8 consecutive elements each,
// and lane l's j-th unit (j = 0, 1) is unit 256 j + l.  A block of 32 is the
// j-th units of FOUR adjacent lanes, block 64 j + l / 4 of the tile, element
// 8 (l % 4) + e of the block.  So the block's largest key is a lane's maximum
// of eight and two DPP exchanges (quad_perm, l ^ 1 and l ^ 2); the butterflies
// of h = 1, 2, 4 run inside a lane's eight registers and h = 8, 16 are those
// two exchanges again — nothing crosses a quad, no ds_swizzle, no
// row_half_mirror.  A unit's codes leave as one b64 (e4m3) or one dword (e2m1)
// store of the lane's own: the nibbles need no neighbour.  A quad's two sign
// words are one Philox call a lane (lane l computes unit j = l % 2's) and two
// DPP broadcasts.  Rounding draws stay keyed by the 4-element group of
// bpsr_cast_sr.h: two calls a unit.  Scale bytes go through LDS and leave as
// b128, as in the f32 kernels.
//
// Ragged tiles and operands off a 16-byte boundary (a 2-byte tensor need only
// be 2-byte aligned) keep the lane map: a unit that is whole and whose operand
// is 16-byte aligned moves as b128, any other element by element, and an
// element past the count is not read, is +0.0, and is not written.
#include "bpsr_cast_sr.h"
#include "bpsr_mx_lanes.h"

namespace bpsr {

namespace {

constexpr uint32_t kHalfTileBytes = kMxTile * 2;
typedef uint32_t u2 __attribute__((ext_vector_type(2)));

// The maximum over the block's four lanes, in every one of them.
__device__ __forceinline__ uint32_t quad_max(uint32_t m) {
  uint32_t o = dpp<kDppXor1>(m);
  m = o > m ? o : m;
  o = dpp<kDppXor2>(m);
  return o > m ? o : m;
}

// One butterfly stage across lanes: `upper` — this lane holds the pair's b.
template <int CTRL>
__device__ __forceinline__ void stage(float (&x)[8], bool upper) {
  const uint32_t flip = upper ? 0x80000000u : 0u;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float other = bitcast<float>(dpp<CTRL>(bitcast<uint32_t>(x[e])));
    x[e] = bitcast<float>(bitcast<uint32_t>(x[e]) ^ flip) + other;
  }
}

// The unnormalised Walsh-Hadamard transform of the block this lane's quad
// holds, h = 1, 2, 4, 8, 16 in this order.
__device__ __forceinline__ void hadamard32(float (&x)[8], uint32_t lane) {
#pragma unroll
  for (int h = 1; h < 8; h <<= 1)
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (!(i & h)) {
        const float a = x[i], b = x[i + h];
        x[i] = a + b;
        x[i + h] = a - b;
      }
  stage<kDppXor1>(x, (lane & 1) != 0);
  stage<kDppXor2>(x, (lane & 2) != 0);
}

// The sign words of the lane's two blocks: block j of the lane is block
// first_block + 64 j + lane / 4 of the tensor.
__device__ __forceinline__ void sign_words(uint32_t first_block, uint32_t lane, uint32_t step,
                                           uint32_t rot_key, uint32_t (&w)[2]) {
  const uint32_t own =
      (uint32_t)philox2x32_10(first_block + (lane & 1) * 64 + lane / 4, step, rot_key);
  w[0] = dpp<0x00>(own);
  w[1] = dpp<0x55>(own);
}

// 0x80000000 where bit 8 (lane % 4) + e of the block's word is set.
__device__ __forceinline__ uint32_t sign_of(uint32_t w, uint32_t lane, int e) {
  return (w >> (8 * (lane & 3) + (uint32_t)e)) << 31;
}

// The f32 bits of a unit's eight elements.
template <int DT>
__device__ __forceinline__ void widen8(const vec16& x, uint32_t (&c)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) c[e] = Wide<DT>::to_f32(Wide<DT>::get(&x, e));
}

// The unit at element p0 of a ragged or misaligned tile.
template <int DT>
__device__ __forceinline__ void load_unit(const unsigned char* g, uint32_t p0, uint32_t count,
                                          bool vec, uint32_t (&c)[8]) {
  if (vec && p0 + 8 <= count) {
    widen8<DT>(ld16<true>(g + (uint64_t)p0 * 2), c);
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    c[e] = 0;
    if (p0 + e < count)
      c[e] = Wide<DT>::to_f32(*reinterpret_cast<const uint16_t*>(g + (uint64_t)(p0 + e) * 2));
  }
}

__device__ __forceinline__ void store_header(unsigned char* payload, uint32_t bits,
                                             uint64_t nelem, uint32_t rotate) {
  vec16 hd;
  hd.w[0] = bits;
  hd.w[1] = (uint32_t)nelem;
  hd.w[2] = (uint32_t)(nelem >> 32);
  hd.w[3] = rotate;
  st16<false>(payload, hd);
}

// A unit's eight codes, w[0] elements 0..3 and w[1] elements 4..7 as encode4 /
// sr_code pack them: one b64 (fp8) or one dword (fp4), cut at the padded end.
template <int BITS>
__device__ __forceinline__ void store_codes(unsigned char* codes, uint32_t p0, uint32_t code_end,
                                            const uint32_t (&w)[2]) {
  if constexpr (BITS == 8) {
    if (p0 < code_end) *reinterpret_cast<u2*>(codes + p0) = u2{w[0], w[1]};
  } else {
    if (p0 / 2 < code_end) *reinterpret_cast<uint32_t*>(codes + p0 / 2) = w[0] | w[1] << 16;
  }
}

// The tile's scale bytes from LDS, cut at the padded end.
__device__ __forceinline__ void store_scales(unsigned char* scales, const unsigned char* sx,
                                             uint32_t lane, uint32_t scale_end) {
  __syncthreads();
  if (lane * 16 < scale_end)
    st16<false>(scales + lane * 16, bitcast<vec16>(*reinterpret_cast<const u4*>(&sx[lane * 16])));
}

// f32 values to a unit of the output type and out: full — the whole tile
// through the descriptor; else a whole unit of an aligned output as b128, any
// other element by element.
template <int DT, int POL>
__device__ __forceinline__ void store_unit(unsigned char* out, uint32_t p0, uint32_t count,
                                           bool vec, bool full, const uint32_t (&o)[8]) {
  vec16 h{};
#pragma unroll
  for (int e = 0; e < 8; ++e) Wide<DT>::put(&h, e, Wide<DT>::from_f32(bitcast<float>(o[e])));
  if (full) {
    const auto ro = __builtin_amdgcn_make_buffer_rsrc(out, 0, kHalfTileBytes, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(h), ro, (int)p0 * 2, 0, kStAux<POL>);
  } else if (vec && p0 + 8 <= count) {
    st16<true>(out + (uint64_t)p0 * 2, h);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (p0 + e < count)
        *reinterpret_cast<uint16_t*>(out + (uint64_t)(p0 + e) * 2) = Wide<DT>::get(&h, e);
  }
}

}  // namespace

template <int DT, int BITS, int POL>
__global__ __launch_bounds__(kBlock) void mx_half_compress_kernel(MxCompress p) {
  __shared__ __attribute__((aligned(16))) unsigned char sx[kMxTileBlocks];
  // grid == nrecs: no bounds test in front of the record load
  const MxRec& r = p.recs[blockIdx.x];
  const unsigned char* const g = r.a;
  unsigned char* const q = r.b;
  const uint32_t seg = r.seg, e0 = r.e0, count = r.count, flags = r.flags;
  unsigned char* const payload = p.segs[seg].payload;
  const uint64_t nelem = p.segs[seg].nelem;
  asm volatile("" ::"s"(g), "s"(q), "s"(e0), "s"(count), "s"(flags), "s"(payload), "s"(nelem));
  const uint32_t lane = threadIdx.x;
  const bool vecg = (flags & kMxVec) != 0, vecq = (flags & kMxVecB) != 0;
  const bool full = vecg && vecq && count == kMxTile;
  auto add = [](uint32_t x, uint32_t y) {
    return bitcast<uint32_t>(bitcast<float>(x) + bitcast<float>(y));
  };
  uint32_t c[2][8];
  if (full) {
    // six b128 a lane, every one issued before the first add
    const auto rg = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(g), 0,
                                                      kHalfTileBytes, 0x00020000);
    const auto rq = __builtin_amdgcn_make_buffer_rsrc(q, 0, kTileBytes, 0x00020000);
    vec16 x[2], y[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int u = (int)vector_of(j, lane);
      x[j] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(rg, u * 16, 0, kLdAux));
      y[j][0] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(rq, u * 32, 0, kLdAux));
      y[j][1] = bitcast<vec16>(__builtin_amdgcn_raw_buffer_load_b128(rq, u * 32 + 16, 0, kLdAux));
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      widen8<DT>(x[j], c[j]);
#pragma unroll
      for (int e = 0; e < 8; ++e) c[j][e] = add(c[j][e], y[j][e >> 2].w[e & 3]);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const uint32_t p0 = vector_of(j, lane) * 8;
      uint32_t gw[8];
      load_unit<DT>(g, p0, count, vecg, gw);
      if (vecq && p0 + 8 <= count) {
        const vec16 y0 = ld16<true>(q + (uint64_t)p0 * 4);
        const vec16 y1 = ld16<true>(q + (uint64_t)p0 * 4 + 16);
#pragma unroll
        for (int e = 0; e < 8; ++e) c[j][e] = add(gw[e], (e < 4 ? y0 : y1).w[e & 3]);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          c[j][e] = 0;
          if (p0 + e < count)
            c[j][e] =
                add(gw[e], *reinterpret_cast<const uint32_t*>(q + (uint64_t)(p0 + e) * 4));
        }
      }
    }
  }
  if (e0 == 0 && lane == 0) store_header(payload, BITS, nelem, 0);
  unsigned char* const scales = payload + kMxHeader + e0 / kMxBlock;
  unsigned char* const codes = payload + mx_codes_at(nelem) + (uint64_t)e0 * BITS / 8;
  // where the tile's codes and scales end, padding included
  const uint32_t code_end = (uint32_t)mx_align16(mx_code_bytes(count, BITS));
  const uint32_t scale_end = (uint32_t)mx_align16(mx_scale_bytes(count));
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t p0 = vector_of(j, lane) * 8;
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t key = c[j][e] & kKeyMask;
      m = key > m ? key : m;
    }
    const uint32_t E = quad_max(m) >> 23;
    const bool bad = E == 255;  // an inf or a NaN in the block
    const uint32_t X = bad ? 255u : (E > MxFmt<BITS>::kEmax ? E - MxFmt<BITS>::kEmax : 0u);
    const float inv = bitcast<float>((254u - (bad ? 127u : X)) << 23), sc = scale_of(X);
    uint32_t w[2];
    vec16 y[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float v[4], f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float t = bitcast<float>(c[j][4 * h + e]) * inv;
        v[e] = bad ? 0.0f
                   : __builtin_fminf(__builtin_fmaxf(t, -MxFmt<BITS>::kMax), MxFmt<BITS>::kMax);
      }
      w[h] = encode4<BITS>(v);
      decode4<BITS>(w[h], f);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        // a non-finite block: d and r' are the NaN in these bits, not a subtract's
        y[h].w[e] =
            bad ? kNaN : bitcast<uint32_t>(bitcast<float>(c[j][4 * h + e]) - f[e] * sc);
      }
    }
    if (full) {
      const auto rq = __builtin_amdgcn_make_buffer_rsrc(q, 0, kTileBytes, 0x00020000);
      __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(y[0]), rq, (int)p0 * 4, 0, kStAux<POL>);
      __builtin_amdgcn_raw_buffer_store_b128(bitcast<u4>(y[1]), rq, (int)p0 * 4 + 16, 0,
                                             kStAux<POL>);
    } else if (vecq && p0 + 8 <= count) {
      st16<false>(q + (uint64_t)p0 * 4, y[0]);
      st16<false>(q + (uint64_t)p0 * 4 + 16, y[1]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (p0 + e < count)
          *reinterpret_cast<uint32_t*>(q + (uint64_t)(p0 + e) * 4) = y[e >> 2].w[e & 3];
    }
    store_codes<BITS>(codes, p0, code_end, w);
    if ((lane & 3) == 0) sx[p0 / kMxBlock] = (unsigned char)X;
  }
  store_scales(scales, sx, lane, scale_end);
}

template <int DT, int BITS, bool ROTATE>
__global__ __launch_bounds__(kBlock) void mx_half_sr_compress_kernel(MxSrCompress p) {
  __shared__ __attribute__((aligned(16))) unsigned char sx[kMxTileBlocks];
  // grid == nrecs: no bounds test in front of the record load
  const MxRec& r = p.recs[blockIdx.x];
  const unsigned char* const g = r.a;
  const uint32_t seg = r.seg, e0 = r.e0, count = r.count, flags = r.flags;
  unsigned char* const payload = p.segs[seg].payload;
  const uint64_t nelem = p.segs[seg].nelem;
  const uint32_t key = p.segs[seg].key, rot_key = p.segs[seg].rot_key, step = p.step;
  asm volatile("" ::"s"(g), "s"(e0), "s"(count), "s"(flags), "s"(payload), "s"(nelem), "s"(key),
               "s"(rot_key), "s"(step));
  const uint32_t lane = threadIdx.x;
  const bool vec = (flags & kMxVec) != 0;
  uint32_t c[2][8];
  if (vec && count == kMxTile) {
    const auto rg = __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(g), 0,
                                                      kHalfTileBytes, 0x00020000);
    vec16 x[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
      x[j] = bitcast<vec16>(
          __builtin_amdgcn_raw_buffer_load_b128(rg, (int)vector_of(j, lane) * 16, 0, kLdAux));
#pragma unroll
    for (int j = 0; j < 2; ++j) widen8<DT>(x[j], c[j]);
  } else {
#pragma unroll
    for (int j = 0; j < 2; ++j) load_unit<DT>(g, vector_of(j, lane) * 8, count, vec, c[j]);
  }
  if (e0 == 0 && lane == 0) store_header(payload, BITS, nelem, ROTATE ? 1u : 0u);
  unsigned char* const scales = payload + kMxHeader + e0 / kMxBlock;
  unsigned char* const codes = payload + mx_codes_at(nelem) + (uint64_t)e0 * BITS / 8;
  // where the tile's codes and scales end, padding included
  const uint32_t code_end = (uint32_t)mx_align16(mx_code_bytes(count, BITS));
  const uint32_t scale_end = (uint32_t)mx_align16(mx_scale_bytes(count));
  uint32_t sw[2] = {0, 0};
  if constexpr (ROTATE) sign_words(e0 / kMxBlock, lane, step, rot_key, sw);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t p0 = vector_of(j, lane) * 8;
    if constexpr (ROTATE) {
      float x[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) x[e] = bitcast<float>(c[j][e] ^ sign_of(sw[j], lane, e));
      hadamard32(x, lane);
      // the block's 32 elements all lie inside the segment
      const bool whole = (p0 & ~(kMxBlock - 1)) + kMxBlock <= count;
#pragma unroll
      for (int e = 0; e < 8; ++e) c[j][e] = whole ? bitcast<uint32_t>(x[e]) : c[j][e];
    }
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const uint32_t k = c[j][e] & kKeyMask;
      m = k > m ? k : m;
    }
    const uint32_t K = quad_max(m), E = K >> 23;
    const bool bad = E == 255;  // an inf or a NaN in the block
    // one more where 2^emax times the largest mantissa would pass the format's max
    const uint32_t Eb = E + ((K & 0x7fffffu) > SrFmt<BITS>::kMant ? 1u : 0u);
    const uint32_t X = bad ? 255u : (Eb > SrFmt<BITS>::kEmax ? Eb - SrFmt<BITS>::kEmax : 0u);
    const float inv = bitcast<float>((254u - (bad ? 127u : X)) << 23);
    uint32_t w[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      // the unit's two Philox groups: 4-element groups 2 u and 2 u + 1 of the tile
      const uint64_t bits =
          philox2x32_10((e0 >> 2) + vector_of(j, lane) * 2 + (uint32_t)h, step, key);
      w[h] = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint32_t v = bitcast<uint32_t>(bitcast<float>(c[j][4 * h + e]) * inv);
        const uint32_t code = sr_code<BITS>(v, (uint32_t)(bits >> (16 * e)) & 0xffffu);
        w[h] |= (bad ? 0u : code) << (e * BITS);
      }
    }
    store_codes<BITS>(codes, p0, code_end, w);
    if ((lane & 3) == 0) sx[p0 / kMxBlock] = (unsigned char)X;
  }
  store_scales(scales, sx, lane, scale_end);
}

// Both folds: P is MxFold (bpsr_k_mx.hip's arithmetic) or MxRhtFold (the
// rotation undone after the sum, bpsr_k_mx_sr.hip's).  Sources are taken kGroup
// at a time: every load of a group is issued ahead of its first add.
template <class P, int DT, int BITS, int POL>
__global__ __launch_bounds__(kBlock) void mx_half_fold_kernel(P p) {
  constexpr bool ROTATE = std::is_same<P, MxRhtFold>::value;
  constexpr int kGroup = 8;
  const MxRec& r = p.recs[blockIdx.x];
  unsigned char* const out = r.a;
  const uint32_t seg = r.seg, e0 = r.e0, count = r.count, flags = r.flags;
  // sizes come from the plan, never from a header
  const uint64_t nelem = p.segs[seg].nelem;
  const int nsrc = p.nsrc;
  asm volatile("" ::"s"(out), "s"(seg), "s"(e0), "s"(count), "s"(flags), "s"(nelem), "s"(nsrc));
  const unsigned char* const* const row = p.srcs + (uint64_t)seg * (uint32_t)nsrc;
  const uint64_t scales_at = kMxHeader + e0 / kMxBlock;
  const uint64_t codes_at = mx_codes_at(nelem) + (uint64_t)e0 * BITS / 8;
  const uint32_t lane = threadIdx.x;
  float acc[2][8];
  bool bad[2] = {false, false};
  for (int s0 = 0; s0 < nsrc; s0 += kGroup) {
    uint32_t w[kGroup][2][2], X[kGroup][2];
#pragma unroll
    for (int k = 0; k < kGroup; ++k) {
      if (s0 + k >= nsrc) break;
      const unsigned char* const src = row[s0 + k];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const uint32_t p0 = vector_of(j, lane) * 8;
        w[k][j][0] = w[k][j][1] = 0;
        X[k][j] = 0;
        // p0 < count: the unit's codes and its block's scale lie inside the payload
        if (p0 < count) {
          if constexpr (BITS == 8) {
            const u2 both =
                __builtin_nontemporal_load(reinterpret_cast<const u2*>(src + codes_at + p0));
            w[k][j][0] = both.x;
            w[k][j][1] = both.y;
          } else {
            const uint32_t both = __builtin_nontemporal_load(
                reinterpret_cast<const uint32_t*>(src + codes_at + p0 / 2));
            w[k][j][0] = both & 0xffffu;
            w[k][j][1] = both >> 16;
          }
          X[k][j] = __builtin_nontemporal_load(src + scales_at + p0 / kMxBlock);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < kGroup; ++k) {
      if (s0 + k >= nsrc) break;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const bool nan = X[k][j] == 255;
        bad[j] = bad[j] || nan;
        const float sc = scale_of(X[k][j]);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          float f[4];
          decode4<BITS>(w[k][j][h], f);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            // the rotated fold marks the block after the sum instead
            const float d = !ROTATE && nan ? bitcast<float>(kNaN) : f[e] * sc;
            acc[j][4 * h + e] = s0 + k == 0 ? d : acc[j][4 * h + e] + d;
          }
        }
      }
    }
  }
  const bool div = p.divisor > 1;
  const float fd = (float)p.divisor;
  const bool vec = (flags & kMxVec) != 0;
  const bool full = vec && count == kMxTile;
  uint32_t sw[2] = {0, 0};
  if constexpr (ROTATE) {
    const uint32_t rot_key = p.segs[seg].rot_key, step = p.step;
    sign_words(e0 / kMxBlock, lane, step, rot_key, sw);
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const uint32_t p0 = vector_of(j, lane) * 8;
    uint32_t o[8];
    if constexpr (ROTATE) {
      float z[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) z[e] = acc[j][e];
      hadamard32(z, lane);
      const bool whole = (p0 & ~(kMxBlock - 1)) + kMxBlock <= count;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float back =
            bitcast<float>(bitcast<uint32_t>(z[e] * 0.03125f) ^ sign_of(sw[j], lane, e));
        const float t = whole ? back : acc[j][e];
        // a source's X == 255 anywhere in the block: the NaN in these bits
        o[e] = bad[j] ? kNaN : bitcast<uint32_t>(div ? t / fd : t);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = bitcast<uint32_t>(div ? acc[j][e] / fd : acc[j][e]);
    }
    store_unit<DT, POL>(out, p0, count, vec, full, o);
  }
}

namespace {

// f(DT, BITS) with the element type and the format as std::integral_constants.
template <class F>
hipError_t half_dispatch(int dtype, uint32_t bits, F&& f) {
  auto with_bits = [&](auto dt) {
    return bits == 8 ? f(dt, std::integral_constant<int, 8>{})
                     : f(dt, std::integral_constant<int, 4>{});
  };
  return dtype == kFloat16 ? with_bits(std::integral_constant<int, kFloat16>{})
                           : with_bits(std::integral_constant<int, kBFloat16>{});
}

template <class P>
hipError_t launch_half_fold(const P& p, int dtype, uint32_t bits, uint64_t out_bytes,
                            const Tuning& tu, hipStream_t s) {
  if (p.nrecs == 0) return hipSuccess;
  const bool wt = cast_store_pol(tu, out_bytes) == kPolWt;
  return half_dispatch(dtype, bits, [&](auto DT, auto B) -> hipError_t {
    constexpr int dt = decltype(DT)::value, b = decltype(B)::value;
    if (wt)
      hipLaunchKernelGGL((mx_half_fold_kernel<P, dt, b, kPolWt>), dim3(p.nrecs), dim3(kBlock), 0,
                         s, p);
    else
      hipLaunchKernelGGL((mx_half_fold_kernel<P, dt, b, kPolNt>), dim3(p.nrecs), dim3(kBlock), 0,
                         s, p);
    return hipGetLastError();
  });
}

}  // namespace

hipError_t launch_mx_half_compress(const MxCompress& p, int dtype, uint32_t bits,
                                   uint64_t resid_bytes, const Tuning& tu, hipStream_t s) {
  if (p.nrecs == 0) return hipSuccess;
  const bool wt = cast_store_pol(tu, resid_bytes) == kPolWt;
  return half_dispatch(dtype, bits, [&](auto DT, auto B) -> hipError_t {
    constexpr int dt = decltype(DT)::value, b = decltype(B)::value;
    if (wt)
      hipLaunchKernelGGL((mx_half_compress_kernel<dt, b, kPolWt>), dim3(p.nrecs), dim3(kBlock), 0,
                         s, p);
    else
      hipLaunchKernelGGL((mx_half_compress_kernel<dt, b, kPolNt>), dim3(p.nrecs), dim3(kBlock), 0,
                         s, p);
    return hipGetLastError();
  });
}

hipError_t launch_mx_half_sr_compress(const MxSrCompress& p, int dtype, uint32_t bits,
                                      bool rotate, hipStream_t s) {
  if (p.nrecs == 0) return hipSuccess;
  return half_dispatch(dtype, bits, [&](auto DT, auto B) -> hipError_t {
    constexpr int dt = decltype(DT)::value, b = decltype(B)::value;
    if (rotate)
      hipLaunchKernelGGL((mx_half_sr_compress_kernel<dt, b, true>), dim3(p.nrecs), dim3(kBlock),
                         0, s, p);
    else
      hipLaunchKernelGGL((mx_half_sr_compress_kernel<dt, b, false>), dim3(p.nrecs), dim3(kBlock),
                         0, s, p);
    return hipGetLastError();
  });
}

hipError_t launch_mx_half_fold(const MxFold& p, int dtype, uint32_t bits, uint64_t out_bytes,
                               const Tuning& tu, hipStream_t s) {
  return launch_half_fold(p, dtype, bits, out_bytes, tu, s);
}

hipError_t launch_mx_half_rht_fold(const MxRhtFold& p, int dtype, uint32_t bits,
                                   uint64_t out_bytes, const Tuning& tu, hipStream_t s) {
  return launch_half_fold(p, dtype, bits, out_bytes, tu, s);
}

}  // namespace bpsr
