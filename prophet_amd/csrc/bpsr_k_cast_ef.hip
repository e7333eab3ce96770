// Error-feedback compress over the fp16 wire (Compression.fp16_ef): the single
// launch and the plan launch of bpsr_cast_ef.h, where the arithmetic, the f32
// scope and the tile's shape are described.  An f32 gradient below 2^-25 is
// sent as zero by the plain fp16 compress every iteration; here it collects in
// the residual until it is worth one fp16 subnormal step.
#include "bpsr_cast_ef.h"

namespace bpsr {

hipError_t launch_compress_ef(void* dst, void* resid, const void* src, size_t nelem,
                              const Tuning& tu, hipStream_t s) {
  return launch_compress_ef_t<NarrowF16>(dst, resid, src, nelem, tu, s);
}

hipError_t launch_cast_plan_ef(const CastRec* table, unsigned char* const* rtab,
                               uint32_t nrecords, int u, uint64_t out_bytes, const Tuning& tu,
                               hipStream_t s) {
  return launch_cast_plan_ef_t<NarrowF16>(table, rtab, nrecords, u, out_bytes, tu, s);
}

}  // namespace bpsr
