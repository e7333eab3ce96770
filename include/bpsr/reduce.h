/*
 * bpsr/reduce.h — C ABI of libbpsr.so, the MI355X (gfx950) gradient-bucket
 * reducer that replaces the host-side CpuReducer of Prophet/BytePS.
 *
 * Every exported name matches `*byteps*`, so it survives the reference's own
 * linker version script (byteps.lds:1-8 exports only *byteps*, *PyInit*,
 * *initc_lib*).  No torch, HIP or C++ types cross this boundary: pointers are
 * device pointers (or host pointers registered/allocated for device access),
 * lengths are BYTES exactly as in the reference, streams are opaque
 * hipStream_t handles passed as void* (NULL = the calling thread's default
 * stream, hipStreamPerThread).
 *
 * Reference interfaces replaced (byteps/common/cpu_reducer.h:41-58):
 *   CpuReducer::sum(void* dst, void* src, size_t len, DataType)      -> byteps_reduce_sum
 *   CpuReducer::sum(void* dst, void* s1, void* s2, size_t, DataType) -> byteps_reduce_sum3
 *   CpuReducer::copy(void* dst, void* src, size_t len)               -> byteps_reduce_copy
 *   the server's per-key fold, byteps/server/server.cc:216-273
 *   (first arrival = accumulator, N-1 SUM_RECV jobs, COPY_MERGED)    -> byteps_reduce_sum_n
 *   one Prophet block of buckets released together
 *   (byteps/common/scheduled_queue.cc:244-296)                       -> byteps_reduce_sum_batched
 *
 * Semantics (bit-exact parity with the compiled reference):
 *   - sum: dst[i] = dst[i] + src[i] for i < len / sizeof(T); the trailing
 *     len % sizeof(T) bytes are NOT touched (cpu_reducer.cc:88).
 *   - fp16: fp32 add then round-to-nearest-even to fp16 after EVERY add
 *     (cpu_reducer.cc:101-125); NaN payload rules of the F16C body for
 *     i < floor(n/8)*8 and 0x7fff for the scalar tail (cpu_reducer.h:77-173).
 *   - integers wrap (two's complement).
 *   - copy: all len bytes (cpu_reducer.cc:209-220).
 *   - sum_n: strict left fold ((s0 + s1) + s2) + ... in the given order.
 *
 * Errors: 0 on success, a negative BYTEPS_REDUCE_E* code otherwise.  Nothing
 * aborts across this ABI (the reference BPS_CHECK-aborts on a bad dtype,
 * cpu_reducer.cc:79-80).  byteps_reduce_last_error() returns a thread-local
 * message for the last failing call on the calling thread.
 *
 * Threading: calls are thread-safe for distinct buffers (the reference calls
 * CpuReducer from BYTEPS_SERVER_ENGINE_THREAD engine threads on distinct
 * keys, server.cc:70-145).  All compute calls are asynchronous on `stream`;
 * byteps_reduce_sync(stream) completes them.
 */
#ifndef BPSR_REDUCE_H
#define BPSR_REDUCE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Only the declarations below leave libbpsr.so: it is compiled with
 * -fvisibility=hidden and linked with the reference's export policy
 * (byteps.lds:1-8, global: *byteps*; local: *). */
#pragma GCC visibility push(default)

/* 3: byteps_server_config.engine_blocking; bpsr/shard.h
 * 4: byteps_server_config.release; byteps_shard_rccl_version
 * 5: byteps_server_create_sized (a caller states its config's size)
 *    additive, still 5: byteps_reduce_compress_fp16 / _decompress_fp16
 *    additive, still 5: byteps_reduce_cast_plan_create / _compress /
 *                       _decompress / _destroy (byteps_cast_desc)
 *    additive, still 5: byteps_reduce_compress_to / _decompress_from /
 *                       byteps_reduce_cast_plan_create_wire (bf16 wire)
 *    additive, still 5: byteps_reduce_compress_ef / _cast_plan_create_ef
 *                       (byteps_cast_ef_desc: error-feedback compression)
 *    additive, still 5: byteps_reduce_compress_sr / _cast_plan_create_sr /
 *                       _cast_plan_compress_sr (byteps_cast_sr_desc:
 *                       stochastic-rounding compression)
 *    additive, still 5: byteps_reduce_cast_plan_decompress_stats (the
 *                       decompress that also reports each segment's sum of
 *                       squares and non-finite count)
 *    additive, still 5: byteps_reduce_cast_plan_measure / byteps_reduce_clip_record /
 *                       byteps_reduce_cast_plan_decompress_scaled
 *                       (byteps_clip_record: clip by global norm and unscale
 *                       inside the decompress)
 *    additive, still 5: byteps_reduce_cast_plan_create_sgd / _cast_plan_apply_sgd
 *                       (byteps_cast_sgd_desc, byteps_sgd_hyper: the SGD step
 *                       inside the decompress) */
#define BYTEPS_REDUCE_ABI_VERSION 5

/* Data type ids: byteps/common/common.h:52-65 (mshadow order), plus bf16 as a
 * build extension (the reference has none). */
enum byteps_reduce_dtype {
  BYTEPS_REDUCE_FLOAT32 = 0,
  BYTEPS_REDUCE_FLOAT64 = 1,
  BYTEPS_REDUCE_FLOAT16 = 2,
  BYTEPS_REDUCE_UINT8 = 3,
  BYTEPS_REDUCE_INT32 = 4,
  BYTEPS_REDUCE_INT8 = 5,
  BYTEPS_REDUCE_INT64 = 6,
  BYTEPS_REDUCE_BFLOAT16 = 11
};

/* Rounding mode for the 16-bit float types (ignored for the others). */
enum byteps_reduce_mode {
  /* Round to the storage type after every pairwise add: bit-exact with the
   * reference CpuReducer fold.  Default. */
  BYTEPS_REDUCE_MODE_REFERENCE = 0,
  /* Widen every input to fp32 once, fold in fp32, narrow once.  Not the
   * reference's arithmetic, but just as deterministic, per element:
   *  - a strict left fold in source order, each add an IEEE fp32 add (round to
   *    nearest even, subnormals kept), then ONE round-to-nearest-even narrowing
   *    to the storage type (overflow gives Inf, subnormals kept);
   *  - NaN: an add whose result is NaN yields the accumulator's NaN if it is
   *    one, else the source's, quieted, sign and payload kept (an fp16 payload
   *    sits in the top 10 fraction bits of the fp32 one); inf + -inf yields the
   *    default NaN with the sign set (fp16 0xfe00, bf16 0xffc0).  The fp16
   *    tail rule of reference mode (0x7fff) does not apply;
   *  - n = 1 is a byte copy (a signalling NaN stays as it is), in
   *    byteps_reduce_sum_n and in every table;
   *  - n > BYTEPS_REDUCE_MAX_SRCS (byteps_reduce_sum_n only): the first 32
   *    sources fold and narrow; each further launch folds the running result
   *    with the next 31 and narrows again.
   * The result is within 1/2 ulp of the fp32 fold.  It is close to the exact
   * sum only where the fp32 partial sums do not cancel: fp16 65504, 1e-4,
   * -65504 folds to 0, although the exact sum 1e-4 is representable. */
  BYTEPS_REDUCE_MODE_ACCUM_F32 = 1
};

enum byteps_reduce_status {
  BYTEPS_REDUCE_OK = 0,
  BYTEPS_REDUCE_EDTYPE = -1,   /* unsupported data type                      */
  BYTEPS_REDUCE_EARGS = -2,    /* bad pointer / count / overlap / mode        */
  BYTEPS_REDUCE_EHIP = -3,     /* HIP runtime error (launch, copy, event)     */
  BYTEPS_REDUCE_ERCCL = -4,    /* collective error (reserved for shard APIs)  */
  BYTEPS_REDUCE_ETIMEOUT = -5, /* a block queue launch gave up on a release   */
  BYTEPS_REDUCE_ECANCELED = -6 /* a queued server pull dropped at shutdown    */
};

/* Most sources one kernel launch folds; byteps_reduce_sum_n chains launches
 * for more (still a strict left fold). */
#define BYTEPS_REDUCE_MAX_SRCS 32

/* One bucket of a batched (Prophet block) reduction: dst = fold(srcs[0..n-1]).
 * dst may alias srcs[0]. */
typedef struct byteps_bucket_desc {
  void* dst;
  const void* srcs[BYTEPS_REDUCE_MAX_SRCS];
  size_t len;   /* bytes */
  int n;        /* 1 <= n <= BYTEPS_REDUCE_MAX_SRCS */
  int reserved;
} byteps_bucket_desc;

/* Library version (BYTEPS_REDUCE_ABI_VERSION). */
int byteps_reduce_version(void);

/* Optional eager initialisation for `device` (hipSetDevice + kernel warm-up);
 * every other call initialises lazily on the current device. */
int byteps_reduce_init(int device);
int byteps_reduce_shutdown(void);

/* CpuReducer::sum(dst, src, len, dtype), cpu_reducer.cc:57-83. */
int byteps_reduce_sum(void* dst, const void* src, size_t len, int dtype, void* stream);

/* CpuReducer::sum(dst, src1, src2, len, dtype), cpu_reducer.cc:130-162.  When
 * both operands are NaN the result is src1's, quieted; FLOAT16 gives src2's,
 * as the compiled reference does.
 *
 * Aliases.  The reference's loops are element-wise, so operands that are the
 * same buffer are legal there, and they are here: byteps_reduce_sum accepts
 * src == dst (dst doubles), byteps_reduce_sum3 accepts dst == src1,
 * dst == src2, src1 == src2 and all three equal, and the result is what
 * separate copies of the same values give.  Only an exact alias is accepted:
 * a dst that overlaps a source partially is EARGS, and nothing is written.
 * For FLOAT16 with both operands NaN, byteps_reduce_sum3(dst, dst, b) keeps
 * b's NaN and byteps_reduce_sum3(dst, a, dst) keeps dst's own: src2's in both,
 * quieted (elements of the scalar tail, from floor(n / 8) * 8 on, give 0x7fff
 * for every NaN). */
int byteps_reduce_sum3(void* dst, const void* src1, const void* src2, size_t len,
                       int dtype, void* stream);

/* Fused N-way left fold: dst = ((srcs[0] + srcs[1]) + ...) + srcs[n-1].
 * dst may alias srcs[0] exactly (the server's zero-copy accumulator,
 * server.cc:216-218); partial overlaps are rejected.  Trailing bytes
 * (len % sizeof(T)) of dst are copied from srcs[0]. */
int byteps_reduce_sum_n(void* dst, const void* const* srcs, int n, size_t len,
                        int dtype, int mode, void* stream);

/* One launch for a whole block of buckets (all of one dtype). */
int byteps_reduce_sum_batched(const byteps_bucket_desc* buckets, int nbuckets,
                              int dtype, int mode, void* stream);

/* A reusable batched reduction: the bucket table of one Prophet block is
 * validated and uploaded to the device once (at plan creation, on the current
 * device); every launch is then ONE kernel with no host work, no allocation
 * and no synchronisation, so it can be captured into a hipGraph.  The reference
 * keys, partitions and server receive buffers are fixed after InitTensor
 * (operations.cc:219-316), so a block's table is fixed across iterations. */
typedef struct byteps_reduce_plan byteps_reduce_plan;
int byteps_reduce_plan_create(const byteps_bucket_desc* buckets, int nbuckets, int dtype,
                              int mode, byteps_reduce_plan** plan);
int byteps_reduce_plan_launch(byteps_reduce_plan* plan, void* stream);
int byteps_reduce_plan_destroy(byteps_reduce_plan* plan);

/* Persistent block consumer: the buckets of one training iteration, grouped
 * into Prophet blocks in release order (block i = buckets
 * [block_end[i-1], block_end[i]), block_end[nblocks-1] == nbuckets), folded by
 * ONE resident kernel per iteration instead of one launch per block.  The
 * kernel takes tiles in table order and starts a block's tiles once that block
 * and every block before it are released, so a block is folded as soon as its
 * pushes have landed — no per-block launch, no per-block drain.  It replaces
 * the per-block release loop of scheduled_queue.cc:244-296 followed by one
 * reduce call per released partition.
 *
 *   launch(q, s)           enqueue the iteration's consumer on stream s;
 *   release(q, b, s)       mark block b released once the work queued before it
 *                          on stream s (e.g. the block's H2D pushes) has
 *                          completed; b < 0 releases every block;
 *   release_range(q, f, c, s)  the same for blocks [f, f + c) in ONE kernel
 *                          (a Prophet release group spanning several blocks);
 *   status(q, s)           synchronise s and report whether a launch gave up:
 *                          a workgroup that waits longer than the timeout
 *                          (default 2 s) for a release sets a sticky error, every
 *                          workgroup then stops and status returns
 *                          BYTEPS_REDUCE_ETIMEOUT (and clears it).
 *
 * Iterations are numbered by epochs (host call order): launch k waits for the
 * k-th release of every block (its release word >= k), so nothing is re-armed
 * between iterations, a block may be released before or after its
 * iteration's launch, and later iterations can be enqueued at once (the
 * caller keeps iteration k + 1's data from landing before launch k consumed
 * the buffers).  Every block must be released once per iteration.  After
 * ETIMEOUT, status() counts the abandoned iteration's missing releases as
 * given.  A launch captured into a hipGraph replays with its epoch fixed, so a
 * capture must release every block before the launch (EARGS otherwise).  One
 * launch of a queue at a time.  Launch and release may be called from
 * different threads.  Table residency as for plans (buffers fixed after
 * InitTensor).  When
 * a block's data lands after the launch, its buffers should not share a 128-B
 * line with an earlier block's (a line read for the earlier block may be
 * cached ahead of the later block's DMA).
 *
 * Live releases need the consumer and the releasing stream on DIFFERENT
 * hardware queues: HIP multiplexes streams onto a few in-order hardware queues
 * per process (GPU_MAX_HW_QUEUES, 4 by default), and a release queued behind
 * the running consumer in a shared queue cannot run until the consumer gives
 * up (timeout, ETIMEOUT; the grid always drains).  Stream priority does not
 * guarantee separate queues (measured), so the consumer always runs on the
 * library's consumer stream for the device — an all-CU-masked stream, which
 * the runtime gives a hardware queue of its own (byteps_reduce_blockq_stream).
 * Launching on that stream costs nothing extra and orders launches and status
 * calls there (work on other streams that reads the outputs must then wait for
 * it, e.g. on an event recorded there); launching on any other stream forks
 * onto it and joins back
 * (two events — ~0.14 ms per iteration at config 3, so launch on the consumer
 * stream when iterations run back to back).  The join-back is queued on the
 * launch stream once EVERY block of the launch's epoch has been released (by
 * the release call that completes the epoch, stream or host), or at
 * byteps_reduce_blockq_join / status, whichever comes first (round 6): a wait
 * for the consumer queued at launch time would sit in the launch stream's
 * in-order hardware queue, which HIP shares with other streams, ahead of any
 * release (or the copies before it) queued later on one of them — the
 * consumer would wait for a release that waits for the consumer, until the
 * timeout (false dependencies).  So work queued on the launch
 * stream after the launch is ordered after the fold only once the epoch is
 * fully released; call join before that if it must be.  The launch stream
 * must outlive that point.  A launch inside a hipGraph
 * capture stays on the capturing stream (pre-released by rule).  Releases on
 * the launch stream itself, before the launch, are always safe.
 * The consumer queues are blocking streams (HIP gives an explicit CU mask only
 * to those), so work on the legacy NULL stream waits for a running consumer —
 * and holds back every stream sharing the NULL stream's hardware queue: do not
 * queue work on the NULL stream between a live launch and its last release
 * (torch: make the current stream a non-default one).
 * Likewise on the host: between a live launch and its last release, the
 * thread that issues the releases must not block on the device
 * (hipDeviceSynchronize, hipFree — including byteps_reduce_blockq_destroy or
 * plan_destroy of another object — or a synchronous copy): the consumer is
 * waiting for the releases that thread has not issued yet. */
typedef struct byteps_reduce_blockq byteps_reduce_blockq;
int byteps_reduce_blockq_create(const byteps_bucket_desc* buckets, int nbuckets,
                                const int* block_end, int nblocks, int dtype, int mode,
                                byteps_reduce_blockq** q);
/* Consumer shape: wg_per_cu = 0 (default) dispatch-ordered — one workgroup
 * per tile, each gated on the release words of the blocks up to its own;
 * 1..8 persistent workgroups per CU sweeping the table; < 0 keeps.  Release
 * timeout in seconds (<= 0 keeps). */
int byteps_reduce_blockq_config(byteps_reduce_blockq* q, int wg_per_cu, double timeout_s);
int byteps_reduce_blockq_launch(byteps_reduce_blockq* q, void* stream);
int byteps_reduce_blockq_release(byteps_reduce_blockq* q, int block, void* stream);
int byteps_reduce_blockq_release_range(byteps_reduce_blockq* q, int first, int count,
                                       void* stream);
int byteps_reduce_blockq_status(byteps_reduce_blockq* q, void* stream);
int byteps_reduce_blockq_destroy(byteps_reduce_blockq* q);
/* Host releases (data already visible to the device, e.g. landed by RDMA into
 * HBM or written by finished device work): after
 * byteps_reduce_blockq_host_releases(q, 1), every launch carries one helper
 * workgroup that forwards release words written by the HOST into the device
 * words, and byteps_reduce_blockq_release_host(q, f, c) releases blocks
 * [f, f + c) with a store to pinned host memory — no stream, no kernel, no
 * copy per release (a release kernel running beside the consumer costs it
 * ~0.4 us each).  The caller guarantees the blocks' data is
 * complete and visible before the call; epochs, timeout and status as above;
 * stream releases may still be mixed in.  Dispatch-ordered consumer only
 * (wg_per_cu = 0); not with a captured launch.  on = 0 turns it off for later
 * launches. */
int byteps_reduce_blockq_host_releases(byteps_reduce_blockq* q, int on);
int byteps_reduce_blockq_release_host(byteps_reduce_blockq* q, int first, int count);
/* The device's consumer stream (see above); owned by the library. */
int byteps_reduce_blockq_stream(byteps_reduce_blockq* q, void** stream);
/* The device's release stream (round 6): a hardware queue of its own, owned
 * by the library, on a different compute pipe than every consumer queue.  A
 * queue that shares a pipe with a running consumer is served ~2x slower (its
 * release kernels took 43 us median instead of 5 beside config 3's consumer,
 * DESIGN.md §4.4 "pipes"), and which pipe a caller's stream lands on is the
 * runtime's choice; the library places its own queues by their HSA ids.
 * Queue a block's pushes (e.g. its H2D copies) and its stream release here,
 * or fork here with an event.  Like the consumer queues it is a blocking
 * stream (see above: no NULL-stream work between a launch and its last
 * release). */
int byteps_reduce_blockq_release_stream(byteps_reduce_blockq* q, void** stream);
/* Diagnostics: the HSA queue ids of the device's consumer queues 0-2 (0 for one
 * not made yet) and of its release queue; returns 4 (needs cap >= 4). */
int byteps_reduce_blockq_queue_ids(byteps_reduce_blockq* q, uint64_t* ids, int cap);
/* Overlap (on = 1; dispatch-ordered consumer only, EARGS otherwise):
 * consecutive launches may run at once, so one iteration's first blocks fold
 * while the previous one's last tiles drain.  A launch goes to whichever of
 * the device's two consumer queues the device's previous block-queue launch
 * did not use, and its first workgroup is dispatched only after every
 * workgroup of that previous launch has started (so waiting workgroups never
 * hold the slots an earlier launch still needs).  The launch
 * forks from `stream` unless `stream` is a consumer queue, and does NOT order
 * `stream` after the fold: byteps_reduce_blockq_join(q, s) makes s wait, on
 * the device, for every block-queue launch of the device so far (status
 * joins first).  Read outputs, or rewrite inputs, only after a join.  on = 0
 * restores the default for later launches. */
int byteps_reduce_blockq_overlap(byteps_reduce_blockq* q, int on);
int byteps_reduce_blockq_join(byteps_reduce_blockq* q, void* stream);
/* Debug (synchronises the device): out = launch epoch, nblocks, the sticky
 * error word, the host's release epoch per block, the device release words,
 * the device block_first table (nblocks + 1), and 1 if the device tile table
 * still equals what was uploaded.  Returns the count written (needs
 * cap >= 4 + 3 * nblocks). */
int byteps_reduce_blockq_debug(byteps_reduce_blockq* q, uint32_t* out, int cap);

/* CpuReducer::copy(dst, src, len), cpu_reducer.cc:209-220 (device to device). */
int byteps_reduce_copy(void* dst, const void* src, size_t len, void* stream);

/* FP16 gradient compression (byteps/torch/compression.py, FP16Compressor):
 * the cast before a push and the cast back after the pull, device to device.
 * `nelem` is in ELEMENTS — the one exception to "lengths are bytes", because
 * the two operands differ in element size (fp16: 2 * nelem bytes; the other:
 * nelem * sizeof(T)).  T (`src_dtype` / `dst_dtype`) is FLOAT32, FLOAT64 or
 * BFLOAT16; anything else is EDTYPE.
 *   compress:    dst[i] = fp16(src[i]), round to nearest even (subnormal
 *                results kept, |x| >= 65520 -> +-inf, signed zeros kept);
 *                f64 is rounded to f32 first, as the host conversion does;
 *                bf16 is widened exactly.  A NaN gives a NaN (payload
 *                unspecified).
 *   decompress:  dst[i] = T(src[i]) for divisor 1 (exact for f32 / f64, RNE
 *                for bf16); for divisor d > 1,
 *                dst[i] = T(fp16(float(src[i]) / float(d))): the quotient is
 *                rounded to fp16 BEFORE it is widened, because the
 *                reference's average divides the compressed tensor in place
 *                (byteps/torch/ops.cc:77-81) and decompresses afterwards.
 * The two byte ranges must not overlap at all, divisor >= 1 (EARGS
 * otherwise); nelem == 0 succeeds without a launch. */
int byteps_reduce_compress_fp16(void* dst, const void* src, size_t nelem, int src_dtype,
                                void* stream);
int byteps_reduce_decompress_fp16(void* dst, const void* src, size_t nelem, int dst_dtype,
                                  int divisor, void* stream);

/* The same casts with the 2-byte wire format named: `wire_dtype` FLOAT16 is
 * exactly the two calls above (same kernels, same checks), BFLOAT16 is bf16
 * gradient compression, whose T is FLOAT32, FLOAT64 or FLOAT16.  Any other
 * pair, T equal to the wire format included, is EDTYPE.  bf16 has f32's
 * exponent range, so a sum of workers' gradients does not overflow where
 * fp16's does at 65,520.
 *   compress:    dst[i] = bf16(src[i]), round to nearest even on f32's upper
 *                16 bits: f32 subnormals are kept, not flushed (0x00008001 ->
 *                0x0001), finite values from 0x7f7f8000 up give +-inf, signed
 *                zeros are kept; f64 is rounded to f32 first (f32 subnormals
 *                produced), f16 is widened exactly.  A NaN gives a NaN
 *                (payload unspecified).
 *   decompress:  dst[i] = T(src[i]) for divisor 1 (exact for f32 / f64; RNE
 *                with overflow to +-inf and fp16 subnormals for f16); for
 *                divisor d > 1, dst[i] = T(bf16(float(src[i]) / float(d))),
 *                the quotient rounded to bf16 BEFORE it is widened.  The
 *                quotient may be an f32 subnormal; it is not flushed.
 * Lengths, overlap, divisor and nelem == 0 as above. */
int byteps_reduce_compress_to(void* dst, const void* src, size_t nelem, int src_dtype,
                              int wire_dtype, void* stream);
int byteps_reduce_decompress_from(void* dst, const void* src, size_t nelem, int dst_dtype,
                                  int wire_dtype, int divisor, void* stream);

/* Cast plan: the casts of a whole push_pull iteration — every gradient to
 * fp16 before the pushes, every result back after the pulls — as ONE launch
 * each way.  Segment i pairs `nelem` elements of the plan's wide type
 * (`wide_dtype`: FLOAT32, FLOAT64 or BFLOAT16, one per plan; else EDTYPE) at
 * `wide` with as many fp16 values at `half`.  compress writes every `half`
 * from its `wide`, decompress every `wide` from its `half`, with the
 * arithmetic and rounding of byteps_reduce_compress_fp16 / _decompress_fp16
 * per segment: the bytes written are those of one such call per segment.  The
 * divisor is given at the launch, so one plan serves every divisor.
 *   create:  cuts the segments into a table resident in device memory, uploaded
 *            once, on the calling thread's current device.  A null pointer
 *            with nelem > 0 is EARGS; because a plan runs both ways, all
 *            2 * nsegs byte ranges must be pairwise disjoint (EARGS).
 *            Segments with nelem == 0 are skipped; a plan without a live
 *            segment is valid and its launches succeed without a launch.
 *   compress / decompress: asynchronous on `stream`; divisor < 1 is EARGS.
 *   destroy: frees the table with hipFree, which waits for launches in flight.
 *   create_wire: a plan whose 2-byte side is `wire_dtype`: FLOAT16 is create
 *            itself, BFLOAT16 pairs FLOAT32, FLOAT64 or FLOAT16 at `wide` with
 *            bf16 values at `half`, per segment the bytes of
 *            byteps_reduce_compress_to / _decompress_from; other pairs are
 *            EDTYPE.  A plan remembers its wire format: compress, decompress
 *            and destroy serve both kinds.
 * The plan holds raw pointers: the caller keeps the segments' memory alive
 * and in place for as long as the plan is launched. */
typedef struct byteps_cast_desc {
  void* wide;
  void* half;
  size_t nelem; /* ELEMENTS, as in the one-tensor casts */
} byteps_cast_desc;
typedef struct byteps_reduce_cast_plan byteps_reduce_cast_plan;
int byteps_reduce_cast_plan_create(const byteps_cast_desc* segs, int nsegs, int wide_dtype,
                                   byteps_reduce_cast_plan** out);
int byteps_reduce_cast_plan_create_wire(const byteps_cast_desc* segs, int nsegs, int wide_dtype,
                                        int wire_dtype, byteps_reduce_cast_plan** out);
int byteps_reduce_cast_plan_compress(byteps_reduce_cast_plan* plan, void* stream);
int byteps_reduce_cast_plan_decompress(byteps_reduce_cast_plan* plan, int divisor, void* stream);
int byteps_reduce_cast_plan_destroy(byteps_reduce_cast_plan* plan);

/* Error-feedback compression: the compress of the two wire formats with a
 * per-tensor FLOAT32 residual that holds what the 2-byte wire could not carry
 * and is added back before the next cast.  For src of FLOAT32, wire format N
 * (`wire_dtype`: FLOAT16 or BFLOAT16) and the residual r at `resid`, per
 * element and in one pass:
 *   c  = src[i] + r[i]                  IEEE f32 add, RNE, subnormals kept
 *   w  = N(c)                           the arithmetic of byteps_reduce_compress_to
 *   b  = f32(w)                         exact
 *   r' = isfinite(b) ? c - b : +0.0     f32 subtract (exact: b is c in fewer bits)
 *   dst[i] = w, r[i] = r'
 * With r == 0 the bytes at dst are those of byteps_reduce_compress_to (but
 * for src -0.0, which the add turns into +0.0: -0 + +0 = +0); where b
 * is finite f32(w) + r' == c exactly; overflow of the wire format, +-inf and
 * NaN leave r' = +0.0 (bits 0), so a residual never holds a non-finite value.
 * Pinned bit for bit to the same four lines in torch's CPU ops.
 *   Scope: FLOAT32 wide tensors only — the residual is f32, and only an f32
 *   wide side shares its vector layout; any other src_dtype / wide_dtype is
 *   EDTYPE, as is a wire other than FLOAT16 or BFLOAT16.
 *   compress_ef: the three byte ranges (2 * nelem at dst, 4 * nelem at resid
 *            and at src) are pairwise disjoint (EARGS); a null pointer with
 *            nelem > 0 is EARGS; nelem == 0 succeeds without a launch.
 *            Asynchronous on `stream`.
 *   cast_plan_create_ef: a cast plan (above) whose segments carry a residual.
 *            All 3 * nsegs byte ranges are pairwise disjoint (EARGS).  The
 *            plan is the same opaque type: _compress on it runs the
 *            error-feedback compress (per segment the bytes of one
 *            compress_ef, wire and residual), _decompress on it is the plain
 *            decompress of `wire_dtype` and leaves the residuals untouched,
 *            _destroy frees the record table and the residual-pointer table. */
int byteps_reduce_compress_ef(void* dst, void* resid, const void* src, size_t nelem,
                              int src_dtype, int wire_dtype, void* stream);
typedef struct byteps_cast_ef_desc {
  void* wide;
  void* half;
  void* resid;
  size_t nelem; /* ELEMENTS */
} byteps_cast_ef_desc;
int byteps_reduce_cast_plan_create_ef(const byteps_cast_ef_desc* segs, int nsegs, int wide_dtype,
                                      int wire_dtype, byteps_reduce_cast_plan** out);

/* Stochastic-rounding compression: the compress of the two wire formats with
 * round-to-nearest-even replaced by rounding up with a probability equal to
 * the dropped fraction, so that the wire value is right in expectation.  No
 * state: dst[i] is a pure function of (the bits of src[i], key, step, i), with
 * i the element's 0-based index in its tensor (its address plays no part).
 *   Random bits: Philox2x32-10 with multiplier 0xD256D193 and key increment
 *   0x9E3779B9 — ten times { hi, lo = mulhilo32(M, c0); c0, c1 = hi ^ k ^ c1,
 *   lo; k += W } — of the counter (c0 = i >> 2, c1 = step) under k = key;
 *   element i takes r16 = the low (i & 1 == 0) or high half of x0 (i & 2 == 0)
 *   or x1.
 *   BFLOAT16, u the f32 bits: w = (u + r16) >> 16 (no wrap) unless the
 *   exponent field is 0xff, where w is byteps_reduce_compress_to's value (inf
 *   stays inf, a NaN a NaN).  A value bf16 holds is sent unchanged; subnormals
 *   and signed zeros are kept; a finite value above bf16's largest becomes inf
 *   with the probability its position gives; the mean over r16 is exact.
 *   FLOAT16: a = u & 0x7fffffff, e = a >> 23.  e == 0xff: compress_to's value.
 *   a >= 0x47800000 (|x| >= 65536): inf.  Else lo = the fp16 value toward zero
 *   and f = the dropped fraction to 16 bits — e >= 113: lo = (a >> 13) -
 *   0x1c000, f = (a & 0x1fff) << 3; below: m = the 24-bit significand (hidden
 *   bit for e > 0), sh = 126 - max(e, 1), lo = m >> sh, f = ((m << 16) >> sh)
 *   & 0xffff (both 0 from sh = 40) — and h = min(lo + ((f + r16) >> 16),
 *   0x7c00), w = sign | h.  The mean over r16 is exact in fp16's normal range;
 *   in its subnormal range f is a floor, so the mean falls short by at most
 *   2^-16 of a subnormal step.
 *   Scope: FLOAT32 wide tensors only (EDTYPE otherwise, as for a wire other
 *   than FLOAT16 or BFLOAT16); at most 2^34 elements a tensor (EARGS).
 *   compress_sr: dst and src must not overlap (EARGS); a null pointer with
 *            nelem > 0 is EARGS; nelem == 0 succeeds without a launch.
 *            Asynchronous on `stream`.  A caller never reuses (key, step) for
 *            different data if it wants independent bits.
 *   cast_plan_create_sr: a cast plan (above) whose segments carry a key.  All
 *            2 * nsegs byte ranges are pairwise disjoint (EARGS).  The plan is
 *            the same opaque type: _cast_plan_compress_sr(plan, step) writes
 *            per segment the bytes of one compress_sr(key of the segment,
 *            step); _decompress is the plain decompress of `wire_dtype`;
 *            _destroy frees both tables.  _cast_plan_compress (no step) on
 *            such a plan is EARGS, as is _cast_plan_compress_sr on a plan
 *            without keys. */
int byteps_reduce_compress_sr(void* dst, const void* src, size_t nelem, int src_dtype,
                              int wire_dtype, uint32_t key, uint32_t step, void* stream);
typedef struct byteps_cast_sr_desc {
  void* wide;
  void* half;
  size_t nelem; /* ELEMENTS */
  uint32_t key;
} byteps_cast_sr_desc;
int byteps_reduce_cast_plan_create_sr(const byteps_cast_sr_desc* segs, int nsegs, int wide_dtype,
                                      int wire_dtype, byteps_reduce_cast_plan** out);
int byteps_reduce_cast_plan_compress_sr(byteps_reduce_cast_plan* plan, uint32_t step,
                                        void* stream);

/* Decompress statistics: _cast_plan_decompress that also reports, for every
 * segment s of the plan (in the order of the table given to create, segments
 * with nelem == 0 included), two numbers computed from exactly the values v it
 * writes to the segment's `wide` (after the divide and the widening):
 *   stats[2 s]     = the sum of (double)v * (double)v over the FINITE v, added
 *                    up in f64.  Each square is exact (the wide types have at
 *                    most 24 significant bits here); every addition rounds
 *                    once.  The order of the additions is the library's: it
 *                    depends on the plan alone, so two launches over the same
 *                    bytes give the same bits.
 *   stats[2 s + 1] = (double) the number of v that are +inf, -inf or NaN.
 * The bytes written to `wide` are those of _cast_plan_decompress, bit for bit.
 * Any plan (create, create_wire, create_ef, create_sr), as for _decompress.
 *   stats:   device memory, 2 * nsegs doubles, every one of them written by
 *            every call.  A null pointer (nsegs > 0), one that is not 8-byte
 *            aligned, or a range that overlaps any byte range of the plan's
 *            segments is EARGS, as are a null plan and divisor < 1; all before
 *            any launch.  A plan of no segments writes nothing and succeeds.
 *   Asynchronous on `stream`: the decompress, then a small kernel that adds
 *   each segment's per-wave partial sums up.  The partials (64 bytes a record)
 *   belong to the plan: its FIRST statistics call allocates them (hipMalloc,
 *   which may synchronise the device), _destroy frees them, and two statistics
 *   launches of one plan must not run concurrently. */
int byteps_reduce_cast_plan_decompress_stats(byteps_reduce_cast_plan* plan, int divisor,
                                             double* stats, void* stream);

/* Clip by global norm and unscale inside the decompress: three launches that
 * compose on one stream, with no host synchronisation between them.
 *
 * _cast_plan_measure: the statistics of _cast_plan_decompress_stats — the same
 *   rows, bit for bit, of the values the plain decompress WOULD write — from a
 *   launch that reads the 2-byte side only and never touches `wide`.  `stats`,
 *   the errors, the partials and the no-concurrency rule are those of
 *   _cast_plan_decompress_stats.
 *
 * byteps_reduce_clip_record: one small kernel (one workgroup, no atomics) over
 *   `rows`, device memory of 2 * nrows doubles — any concatenation of plans'
 *   statistics rows {sumsq_s, nonfinite_s}.  All f64 unless said:
 *     sumsq     = the sum of rows[s].sumsq, in an order nrows alone fixes
 *     nonfinite = the sum of rows[s].nonfinite, exact
 *     inv       = (double)*inv_scale, or 1.0 for a null inv_scale
 *     norm      = sqrt(sumsq) * inv     (the unscaled gradients' L2 norm over
 *                                        their finite values)
 *     c         = min(1.0, max_norm / (norm + eps))
 *     coef      = (float)c
 *     mult      = (float)(c * inv)
 *   Non-finite values do not enter the norm: they are counted, and the caller
 *   skips the step (GradScaler's found_inf).  nrows == 0 gives sumsq 0, coef 1.
 *   `inv_scale`: device memory, one f32, or null.  `out`: device memory, 32
 *   bytes, 8-byte aligned.  EARGS before any launch: null rows with nrows > 0,
 *   nrows < 0, null or misaligned out, max_norm not > 0 or not finite, eps < 0
 *   (or NaN).
 *
 * _cast_plan_decompress_scaled: _cast_plan_decompress with every written value
 *   v (divided on the 2-byte value, rounded to the wire format, widened)
 *   multiplied by m = *mult, one rounding per wide dtype:
 *     FLOAT32            v * m in f32 (subnormals kept)
 *     BFLOAT16, FLOAT16  the f32 product f32(v) * m, rounded to nearest even
 *     FLOAT64            (double)v * (double)m, which is exact
 *   NaN stays NaN and +-inf stays +-inf for a finite positive m; NaN payloads
 *   are not pinned.  `mult`: device memory, one f32, read by the launch
 *   (typically &record->mult).  EARGS before any launch: a null plan, divisor
 *   < 1, a null mult, one that is not 4-byte aligned or that lies inside any
 *   byte range of the plan's segments.  Any plan, as for _decompress. */
typedef struct byteps_clip_record {
  double sumsq;
  double nonfinite;
  double norm;
  float coef;
  float mult;
} byteps_clip_record;
int byteps_reduce_cast_plan_measure(byteps_reduce_cast_plan* plan, int divisor, double* stats,
                                    void* stream);
int byteps_reduce_clip_record(const double* rows, int nrows, double max_norm, double eps,
                              const float* inv_scale, byteps_clip_record* out, void* stream);
int byteps_reduce_cast_plan_decompress_scaled(byteps_reduce_cast_plan* plan, int divisor,
                                              const float* mult, void* stream);

/* The SGD step inside the decompress: the last pull's result goes straight
 * into the parameters.  An SGD plan's segments name the f32 parameter, the
 * 2-byte wire buffer and the f32 momentum buffer; _apply_sgd is ONE launch
 * that reads all three and writes the parameter and the momentum in place
 * (2 + 4 + 4 bytes read, 4 + 4 written an element).  The gradient is never
 * written.  Per element, every line one IEEE f32 operation, rounded to nearest
 * even, subnormals kept, nothing fused; lr, mu (momentum), wd (weight_decay)
 * and mult are f32:
 *
 *   h  = the wire value; for divisor > 1: wire(f32(h) / divisor), the divide
 *        of _decompress
 *   g  = f32(h)                        exact
 *   g  = g * mult                      only with a record (the rounding of
 *                                      _cast_plan_decompress_scaled)
 *   g  = g + wd * p                    only when wd != 0
 *   m' = mu * m + g
 *   d  = nesterov ? g + mu * m' : m'
 *   p' = p - lr * d
 *
 * The momentum buffer always exists; zeroed, the first step is torch's
 * buf = grad, as values.  mu == 0 follows the formula literally.  NaN payloads
 * are not pinned, NaN-ness is.  Pinned to prophet_amd/sgd.py, which agrees
 * with torch.optim.SGD wherever every product and sum is exact.
 *
 * `rec`: null, or a byteps_clip_record in device memory (typically the one
 * byteps_reduce_clip_record wrote earlier on the same stream); its mult scales
 * the gradient.  With skip_nonfinite != 0 and rec->nonfinite != 0 the launch
 * writes nothing — p and m keep every byte — with no host round trip.
 *
 * _create_sgd: the plan is the opaque cast plan, _destroy frees it.
 *   Parameters and momenta are FLOAT32; wire_dtype is FLOAT16 or BFLOAT16,
 *   anything else EDTYPE.  All 3 * nsegs byte ranges must be pairwise disjoint
 *   and a null pointer with nelem > 0 is EARGS.  On an SGD plan every other
 *   _cast_plan_* call (_compress, _compress_sr, _decompress,
 *   _decompress_stats, _measure, _decompress_scaled) is EARGS: it would write
 *   gradients over parameters.  Measure through a plain plan over the same
 *   wire buffers.
 * _apply_sgd: asynchronous on `stream`; a plan without records succeeds
 *   without a launch.  EARGS before any launch, nothing written: a null plan,
 *   a plan that is not an SGD plan, a null h, divisor < 1, lr not finite,
 *   momentum not in [0, 1) (or NaN), weight_decay < 0 or not finite, nesterov
 *   with momentum == 0, skip_nonfinite with a null rec, a rec that is not
 *   8-byte aligned or that lies inside any byte range of the plan's segments. */
typedef struct byteps_cast_sgd_desc {
  void* param;
  void* half;
  void* momentum;
  size_t nelem;
} byteps_cast_sgd_desc;
int byteps_reduce_cast_plan_create_sgd(const byteps_cast_sgd_desc* segs, int nsegs, int wire_dtype,
                                       byteps_reduce_cast_plan** out);
typedef struct byteps_sgd_hyper {
  float lr, momentum, weight_decay;
  int nesterov;
} byteps_sgd_hyper;
int byteps_reduce_cast_plan_apply_sgd(byteps_reduce_cast_plan* plan, int divisor,
                                      const byteps_sgd_hyper* h, const byteps_clip_record* rec,
                                      int skip_nonfinite, void* stream);

/* Block the calling thread until all work queued on `stream` has finished. */
int byteps_reduce_sync(void* stream);

/* Size in bytes of one element of `dtype` (getDataTypeLength, common.cc:126-143),
 * or BYTEPS_REDUCE_EDTYPE. */
int byteps_reduce_dtype_size(int dtype);

/* Thread-local description of the last error on this thread ("" if none). */
const char* byteps_reduce_last_error(void);

/* Launch tuning (process-wide; defaults chosen from measurements, see
 * DESIGN.md §4.1).  vpt: 16-B vectors per thread per tile (1, 2 or 4);
 * nt: non-temporal loads and stores (0/1); max_grid: grid cap in 256-thread
 * workgroups (tile-stride beyond); occ: workgroups resident per CU, enforced
 * through the dynamic LDS request (0 = hardware limit, 1..8).  A value <= 0
 * (nt, occ: < 0) keeps the current setting.  Also settable through the
 * environment: BPSR_VPT, BPSR_NT, BPSR_MAX_GRID, BPSR_OCC. */
int byteps_reduce_set_tuning(int vpt, int nt, int max_grid, int occ);
int byteps_reduce_get_tuning(int* vpt, int* nt, int* max_grid, int* occ);

#pragma GCC visibility pop

#ifdef __cplusplus
}
#endif
#endif /* BPSR_REDUCE_H */
