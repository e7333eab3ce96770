// Cast plan (byteps_reduce_cast_plan_*): a whole iteration's fp16 casts in one
// launch.  A push_pull iteration compresses every gradient before the pushes
// and decompresses every result after the pulls; one cast_kernel launch per
// tensor (bpsr_k_cast.hip) is all launch cost for a model whose gradients are
// mostly a few KiB.  Here the segments are cut ahead of time into a resident
// table of CastRec records (bpsr_cast_table.cpp), one per workgroup, and
// workgroup b runs record b with the single cast's own per-tile code
// (bpsr_cast_impl.h), so every segment's bytes equal what the one-tensor call
// writes.
//
// The record is 32 bytes read at a wave-uniform address before anything is
// stored: scalar loads, one round trip, and both pointers arrive already
// advanced to the tile.  A full tile builds its two buffer descriptors from
// those scalars, sized to the tile — the hardware drops any access outside it —
// and the guarded tile and the element range read nothing past `count`.  The
// same table serves both directions (the record names the wide and the fp16
// side, COMPRESS picks which is read), and the divisor is a kernel argument:
// one plan, every divisor.  The kernel and its launch are templates on the wire
// format (bpsr_cast_plan.h); this unit instantiates the fp16 wire.
#include "bpsr_cast_plan.h"

namespace bpsr {

hipError_t launch_cast_plan(bool compress, const CastRec* table, uint32_t nrecords,
                            int wide_dtype, int divisor, int u, uint64_t out_bytes,
                            const Tuning& tu, hipStream_t s) {
  return launch_plan<NarrowF16, kBFloat16>(compress, table, nrecords, wide_dtype, divisor, u,
                                           out_bytes, tu, s);
}

}  // namespace bpsr
