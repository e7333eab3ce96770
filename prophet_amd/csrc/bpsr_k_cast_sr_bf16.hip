// Stochastic-rounding compress over the bf16 wire (Compression.bf16_sr): the
// single launch and the plan launch of bpsr_cast_sr.h.  bf16 keeps 8
// significant bits: a gradient of 1 + 2^-12 is sent as 1.0 by the plain
// compress every iteration; here it is sent as 1 + 2^-7 one time in 32.
#include "bpsr_cast_sr.h"

namespace bpsr {

hipError_t launch_compress_sr_bf16(void* dst, const void* src, size_t nelem, uint32_t key,
                                   uint32_t step, const Tuning& tu, hipStream_t s) {
  return launch_compress_sr_t<NarrowBF16>(dst, src, nelem, key, step, tu, s);
}

hipError_t launch_cast_plan_sr_bf16(const CastRec* table, const CastSrRec* stab,
                                    uint32_t nrecords, uint32_t step, int u, uint64_t out_bytes,
                                    const Tuning& tu, hipStream_t s) {
  return launch_cast_plan_sr_t<NarrowBF16>(table, stab, nrecords, step, u, out_bytes, tu, s);
}

}  // namespace bpsr
