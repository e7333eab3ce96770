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
// entirely.  The kernel and its launch are templates on the wire format
// (bpsr_cast_single.h); this unit instantiates the fp16 wire.
#include "bpsr_cast_single.h"

namespace bpsr {

hipError_t launch_compress_fp16(void* dst, const void* src, size_t nelem, int src_dtype,
                                const Tuning& tu, hipStream_t s) {
  return launch_cast<NarrowF16, kBFloat16>(true, dst, src, nelem, src_dtype, 1, tu, s);
}

hipError_t launch_decompress_fp16(void* dst, const void* src, size_t nelem, int dst_dtype,
                                  int divisor, const Tuning& tu, hipStream_t s) {
  return launch_cast<NarrowF16, kBFloat16>(false, dst, src, nelem, dst_dtype, divisor, tu, s);
}

}  // namespace bpsr
