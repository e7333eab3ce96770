// Stochastic-rounding compress over the fp16 wire (Compression.fp16_sr): the
// single launch and the plan launch of bpsr_cast_sr.h, where the random bits,
// the rounding, the f32 scope and the tile's shape are described.  An f32
// gradient below 2^-25 is sent as zero by the plain fp16 compress every
// iteration; here it is sent as one fp16 subnormal step with the probability
// that makes the mean right, and no state is kept.
#include "bpsr_cast_sr.h"

namespace bpsr {

hipError_t launch_compress_sr(void* dst, const void* src, size_t nelem, uint32_t key,
                              uint32_t step, const Tuning& tu, hipStream_t s) {
  return launch_compress_sr_t<NarrowF16>(dst, src, nelem, key, step, tu, s);
}

hipError_t launch_cast_plan_sr(const CastRec* table, const CastSrRec* stab, uint32_t nrecords,
                               uint32_t step, int u, uint64_t out_bytes, const Tuning& tu,
                               hipStream_t s) {
  return launch_cast_plan_sr_t<NarrowF16>(table, stab, nrecords, step, u, out_bytes, tu, s);
}

}  // namespace bpsr
