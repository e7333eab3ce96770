// BF16 gradient compression (Compression.bf16) on the device: the cast to
// bf16 before a push and the cast back after the pull, the latter fused with
// push_pull(average=True)'s divide.  The fp16 wire's kernel (bpsr_k_cast.hip,
// bpsr_cast_single.h) with the other narrow format: the same cut, tiles,
// re-dealt wide side, buffer descriptors, cache policy and residency.
//
//   compress    b[i]   = rne_bf16(float(src[i]))        src: f32, f64 or f16
//   decompress  dst[i] = T(b[i])                         divisor 1
//               dst[i] = T(rne_bf16(float(b[i]) / float(divisor)))   divisor > 1
//
// Pinned bit for bit to torch's CPU casts.  The f32 -> bf16 step is the
// integer round-to-nearest-even of the folds (f32_to_bf16_rne: add 0x7fff and
// the kept half's low bit, shift), not gfx950's packed convert: it rounds the
// bit pattern, so f32 subnormals are kept (0x00008001 -> 0x0001) and values
// from 0x7f7f8000 up carry into inf with no dependence on the wave's denormal
// mode, it is the function the server's bf16 folds are already pinned with,
// and the cast is bound by memory (6 bytes an f32 element), not by these four
// integer instructions.  f64 is rounded to f32 first, as the host conversion
// does (1 + 2^-8 + 2^-40 gives 0x3f80), and that step produces f32 subnormals
// (1e-40 gives 0x0001).  f16 widens exactly.  NaN in, NaN out; the payload is
// not part of the contract.
//
// The divide: the reference divides the COMPRESSED tensor, so the quotient is
// rounded to bf16 before it is widened.  Unlike fp16's, a bf16 quotient can
// leave f32's normal range (for divisor 3, 638 of the 65,536 patterns have a
// non-zero f32-subnormal quotient), so the plain IEEE `/` and the f64 -> f32
// convert rely on f32 denormals being on: the build's default for gfx950
// (no -fgpu-flush-denormals-to-zero, no fast-math; Makefile).
#include "bpsr_cast_single.h"

namespace bpsr {

hipError_t launch_compress_bf16(void* dst, const void* src, size_t nelem, int src_dtype,
                                const Tuning& tu, hipStream_t s) {
  return launch_cast<NarrowBF16, kFloat16>(true, dst, src, nelem, src_dtype, 1, tu, s);
}

hipError_t launch_decompress_bf16(void* dst, const void* src, size_t nelem, int dst_dtype,
                                  int divisor, const Tuning& tu, hipStream_t s) {
  return launch_cast<NarrowBF16, kFloat16>(false, dst, src, nelem, dst_dtype, divisor, tu, s);
}

}  // namespace bpsr
