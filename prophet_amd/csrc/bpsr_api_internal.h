// What the units of the fold C ABI share: bpsr_api.cpp (errors, tuning, the
// fold calls), bpsr_table.cpp (batch tables), bpsr_cast_table.cpp (cast plan
// tables), bpsr_queues.cpp (the devices'
// library queues and dispatch sequence), bpsr_blockq.cpp (block queue) and
// bpsr_keyq.cpp (keyed queue).
#pragma once

#include <mutex>
#include <utility>
#include <vector>

#include "bpsr_internal.h"

namespace bpsr {

// A snapshot of the process-wide tuning (bpsr_api.cpp: tuning_for_n).
Tuning launch_tuning_for_n(int n);

inline hipStream_t stream_of(void* s) {
  return s ? reinterpret_cast<hipStream_t>(s) : hipStreamPerThread;
}

inline bool overlaps_partially(const void* a, const void* b, size_t len) {
  if (a == b || len == 0) return false;
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x < y + len && y < x + len;
}

inline int check_common(int dtype, int mode) {
  if (elem_size(dtype) == 0) return fail(BYTEPS_REDUCE_EDTYPE, "Unsupported data type: %d", dtype);
  if (mode != kModeReference && mode != kModeAccumF32)
    return fail(BYTEPS_REDUCE_EARGS, "unknown mode %d", mode);
  return BYTEPS_REDUCE_OK;
}

// `n` objects (of 32-bit words) in pinned, coherent host memory mapped into
// the device, zeroed word by word with release stores (the device polls such
// words): the host view and the device view.  On failure nothing stays
// allocated and `*step` (optional) names the HIP call that failed.
template <class T>
hipError_t pinned_words(size_t n, T** host, T** dev, const char** step = nullptr) {
  static_assert(sizeof(T) % sizeof(uint32_t) == 0, "whole 32-bit words");
  void *p = nullptr, *d = nullptr;
  if (step) *step = "hipHostMalloc";
  hipError_t e = hipHostMalloc(&p, sizeof(T) * n, hipHostMallocCoherent | hipHostMallocMapped);
  if (e != hipSuccess) return e;
  if (step) *step = "hipHostGetDevicePointer";
  if ((e = hipHostGetDevicePointer(&d, p, 0)) != hipSuccess) {
    (void)hipHostFree(p);
    return e;
  }
  for (size_t i = 0; i < sizeof(T) * n / sizeof(uint32_t); ++i)
    __atomic_store_n(static_cast<uint32_t*>(p) + i, 0u, __ATOMIC_RELEASE);
  *host = static_cast<T*>(p);
  *dev = static_cast<T*>(d);
  return hipSuccess;
}

// ------------------------------------------------ batch tables (bpsr_table.cpp) --
struct TableInfo {
  int vpt = 1;   // tile size of the batched kernel for this table
  int nmax = 1;  // most sources of any bucket (residency rule, tuning_for_n)
  int live = 0;          // buckets with len > 0
  uint32_t tiles = 0;    // workgroups (element tiles first, then vector tiles)
  uint32_t rec_stride = 0;
  size_t recs_off = 0;   // byte offset of the tile records in the table
  size_t bytes = 0;      // bytes to upload
};

// Validate buckets and write [BatchEntry x live][pad to 256][TileRec x tiles]
// into `out` (bpsr_internal.h: TileHead).  With `block_end` (a block queue:
// block i = buckets [block_end[i-1], block_end[i])), the records are laid out
// block by block — each block's element tiles, then its vector tiles — and
// `block_first` receives every block's first record (nblocks + 1 entries).
int build_table(const byteps_bucket_desc* buckets, int nbuckets, int dtype, std::vector<char>& out,
                TableInfo* ti, const int* block_end = nullptr, int nblocks = 0,
                std::vector<uint32_t>* block_first = nullptr, int force_vpt = 0);

// `in_hbm`: the records live in device memory.  A table read zero-copy from
// pinned host staging (batched_with_ring, small tables) is not prefetched:
// host pages are not cached in L2, so the touch would only add a PCIe round
// trip that every workgroup waits for before it retires.
BatchLaunch batch_launch(const void* dev_table, const TableInfo& ti, bool in_hbm = true);

// ------------------------------------ cast tables (bpsr_cast_table.cpp) --
struct CastTableInfo {
  int u = 1;             // tile size: kBlock * u 8-element units (1, 2 or 4)
  int live = 0;          // segments with nelem > 0
  uint32_t records = 0;  // workgroups (guarded tiles and element ranges, then full tiles)
  uint64_t nelem = 0;    // elements of all segments (store policy: the launch's output bytes)
  size_t bytes = 0;      // bytes to upload
};

// The rounding scheme of a cast: what a single compress, a plan and its table
// are made for.  kCastSgd: a plan alone (byteps_reduce_cast_plan_create_sgd),
// whose table is an error-feedback plan's over (parameter, wire, momentum).
enum CastScheme { kCastPlain = 0, kCastEf = 1, kCastSr = 2, kCastSgd = 3 };

// Which wide dtypes travel in which 2-byte wire format, per scheme: fp16
// carries f32, f64 and bf16, bf16 carries f32, f64 and fp16; error feedback
// and stochastic rounding take f32 alone.  Anything else, an unknown wire and
// wide == wire included, is the dtype error.
int cast_dtype_check(int wire, int wide_dtype, CastScheme scheme);

// One operand of a single cast: `nelem` elements of `es` bytes at `p`; `name`
// is what an overlap message calls it.
struct CastOperand {
  const char* name;
  const void* p;
  size_t es;
};
// Every check of a single cast, in this order: the dtypes (cast_dtype_check),
// the divisor (1 for a compress), nelem == 0 (returns 1: nothing to do, null
// pointers allowed), a null operand, the element count (2^34 at most for
// stochastic rounding; no byte count may overflow), an operand that wraps the
// address space, and any two of the `n` operands overlapping.  No HIP call.
int cast_check(int wire, int wide_dtype, CastScheme scheme, int divisor, size_t nelem,
               const CastOperand* ops, int n);

// Every segment's records, in CSR form (the decompress statistics'
// finish kernel adds a segment's partials up from it): segment s of the
// caller's table owns records seg_recs[seg_begin[s] .. seg_begin[s + 1]),
// ascending; a segment with nelem == 0 owns none.  seg_begin has nsegs + 1
// entries, seg_recs one per record.  `ranges`: the byte range of every operand
// of every non-empty segment, ascending by first byte (the statistics' output
// must stay clear of them).
struct CastSegList {
  std::vector<uint32_t> seg_begin;
  std::vector<uint32_t> seg_recs;
  std::vector<std::pair<uintptr_t, uintptr_t>> ranges;
};

// Validate the segments (null pointers, pairwise disjoint byte ranges, grid
// size) and write [CastRec x records] into `out` (bpsr_internal.h: CastRec);
// on an error every output is left as it was.  Every segment is cut as a
// single cast is (cast_cut); the tile size is the single cast's rule applied
// to the whole launch: `copy_vpt` (Tuning::copy_vpt), halved while the launch
// would have fewer than kMinTiles vector tiles.  `lists`, where it is not
// null, is filled too; the table and the parallel arrays are byte for byte
// the same with and without it.  No HIP call.
int build_cast_table(const byteps_cast_desc* segs, int nsegs, int wide_dtype, int copy_vpt,
                     std::vector<char>& out, CastTableInfo* ti, CastSegList* lists = nullptr);
// The same for an error-feedback plan (wide_dtype FLOAT32, else EDTYPE): the
// cut also asks the residual to co-align (cast_cut_ef), all 3 * nsegs byte
// ranges must be pairwise disjoint, a null residual with nelem > 0 is EARGS,
// and `resid_out` receives one pointer per record: the segment's residual
// plus (the record's wide pointer - the segment's wide pointer).
int build_cast_table_ef(const byteps_cast_ef_desc* segs, int nsegs, int wide_dtype, int copy_vpt,
                        std::vector<char>& out, std::vector<unsigned char*>& resid_out,
                        CastTableInfo* ti, CastSegList* lists = nullptr);
// The same for a stochastic-rounding plan (wide_dtype FLOAT32, else EDTYPE):
// the cut is the plain one (cast_cut), the 2 * nsegs byte ranges must be
// pairwise disjoint, a segment of more than 2^34 elements is EARGS, the
// records are byte for byte build_cast_table's, and `sr_out` receives one
// entry per record: the index in its segment of the record's first element
// and the segment's key.
int build_cast_table_sr(const byteps_cast_sr_desc* segs, int nsegs, int wide_dtype, int copy_vpt,
                        std::vector<char>& out, std::vector<CastSrRec>& sr_out,
                        CastTableInfo* ti, CastSegList* lists = nullptr);

// ------------------------------------- library queues (bpsr_queues.cpp) --
// Per device, created on first use, never destroyed: the four library queues
// (all-CU-masked streams, each a hardware queue of its own; queue 0 is
// byteps_reduce_blockq_stream, where every launch without overlap runs, in
// launch order; queue 1 the overlapped launches' second queue; queue 2 the
// PS server's keyed consumers, so that a block-queue join never waits for a
// keyed epoch that waits for host releases; queue 3 the release queue,
// byteps_reduce_blockq_release_stream) and the dispatch sequence every
// block-queue launch outside a capture takes part in (DESIGN.md §4.4, round
// 5): sequence numbers, the started-workgroup counter and its target, the
// signal word, the stream of the latest launch, and per stream the completion
// event of its latest launch (what byteps_reduce_blockq_join waits for).
constexpr int kReleaseQueue = 3, kLibraryQueues = 4;
struct ConsumerDev {
  std::mutex mu;                        // sequence order = enqueue order
  hipStream_t q[kLibraryQueues] = {nullptr, nullptr, nullptr, nullptr};
  // Placement (round 6, DESIGN.md §4.4 "pipes"): the HSA ids of the queues,
  // and queues made while placing them that did not fit (kept, idle: a
  // destroyed queue would reshuffle the hardware's queue map).
  uint64_t qid[kLibraryQueues] = {0, 0, 0, 0};
  std::vector<std::pair<hipStream_t, uint64_t>> spare;
  uint64_t* idw = nullptr;              // pinned word read_queue_id writes (host view)
  uint64_t* idw_dev = nullptr;          // ... its device view
  unsigned long long* started = nullptr;  // started counter (device, a line of its own)
  unsigned long long target = 0;        // counted workgroups of every launch so far
  hipStream_t last = nullptr;           // stream of the latest launch
  bool any = false;                     // a launch is in the sequence
  struct Tail {
    hipStream_t stream;
    hipEvent_t ev;
    bool record;  // the latest launch there carried no stop event: join records one
  };
  std::vector<Tail> tails;
};

// The device's entry; null, with the error set (EARGS), for a device number
// the library has no entry for.
ConsumerDev* consumer_dev(int device);
// Library queue `k` of the device (the set is made on first use): 0 every
// launch without overlap, 1 the overlapped launches' second queue, 2 keyed
// consumers, kReleaseQueue the release queue — a hardware queue on a pipe no
// consumer queue uses.
hipError_t library_queue(int device, int cus, int k, hipStream_t* out);
// The HSA ids of the device's library queues (0: not made yet).
void library_queue_ids(const ConsumerDev* D, uint64_t ids[kLibraryQueues]);
// D.mu held (all three): the join entry of a stream, and a launch's place in
// the device's dispatch sequence before and after its kernel is enqueued.
hipError_t seq_tail(ConsumerDev& D, hipStream_t s, ConsumerDev::Tail** out);
hipError_t seq_prepare(ConsumerDev& D, int device, BlockqLaunch& Q, hipStream_t ls,
                       uint64_t gate_ticks);
void seq_commit(ConsumerDev& D, const BlockqLaunch& Q, hipStream_t ls);

}  // namespace bpsr

// ----------------------------------------------- block queue (bpsr_blockq.cpp) --
struct byteps_reduce_blockq {
  int device = 0;
  int dtype = 0;
  int mode = 0;
  int nblocks = 0;
  int occ = 0;               // 0: dispatch-ordered; > 0: persistent workgroups per CU
  int gate_occ = 2;          // dispatch-ordered: resident workgroups per CU, at most
  int cus = 0;
  double timeout_s = 2.0;
  uint64_t clock_khz = 0;    // wall_clock64() rate
  void* dev_table = nullptr; // BatchEntry table + tile records
  uint32_t* flags = nullptr; // [nblocks] release words, then [nblocks + 1] block_first
  bpsr::BlockqCtl* ctl = nullptr;
  uint32_t* host_err = nullptr;  // pinned word for blockq_status
  bpsr::TableInfo ti;
  // Epochs (host call order): launch k consumes epoch k; the k-th release of
  // block b carries epoch k.  Guarded: launches and releases may come from
  // different threads (a transport's receive threads release blocks).
  std::mutex mu;
  uint32_t launch_epoch = 0;
  std::vector<uint32_t> rel_epoch;  // per block: epoch of its latest release
  std::vector<char> host_table;     // what was uploaded (byteps_reduce_blockq_debug)
  // The consumer runs on the device's consumer stream (an explicit all-CU
  // mask: the runtime gives such a stream a hardware queue of its own),
  // forked from and joined into the caller's stream unless the caller
  // launches on that stream itself.  A live release must never sit behind
  // the spinning consumer in a shared in-order hardware queue, and stream
  // priority alone does not guarantee separate queues (measured: torch's
  // pooled high- and normal-priority streams shared one for some pool
  // indices, tools/pushloop_diag.py).
  bool own_queue = true;
  // Overlap (byteps_reduce_blockq_overlap): launches
  // alternate between the device's two consumer queues and do not join back.
  bool overlap = false;
  hipEvent_t fork_ev = nullptr;
  // Deferred join-back (round 6, DESIGN.md §4.4 "false dependencies"): a
  // launch forked from the caller's stream `s` (no overlap) makes `s` wait
  // for its consumer only once every block of its epoch has been released
  // (or at join / status).  A wait queued on `s` at launch time sits in the
  // in-order hardware queue `s` shares with other streams, and a release (or
  // the copies before it) queued on one of those streams would then wait
  // behind the very consumer it releases: a stall until the timeout (r05s76,
  // measured r06s02).  Each such launch completes an event of its own.
  struct PendingJoin {
    hipStream_t s;
    hipEvent_t ev;
    uint32_t epoch;
  };
  std::vector<PendingJoin> pend_join;  // under mu
  std::vector<hipEvent_t> join_evs;    // free events (under mu)
  // Host releases (byteps_reduce_blockq_host_releases): pinned, coherent
  // words the host writes and the launch's helper workgroup forwards.
  uint32_t* hflags = nullptr;
  uint32_t* hflags_dev = nullptr;
  bool host_rel = false;
  // Keyed queue (bpsr::keyq_*, the PS server's device releases): one block
  // per key, (arrival order << 32 | epoch) words, the control word in pinned
  // host memory so the server reads a timeout without a copy.
  bool keyed = false;
  bool wide = false;                // 9..16 sources: a second word per block (positions 8..15)
  uint64_t* kwords = nullptr;       // device, one per block [+ the second words after them]
  uint64_t* khwords = nullptr;      // pinned host, two per block (epoch parity) [+ second words]
  uint64_t* khwords_dev = nullptr;
  bpsr::BlockqCtl* hctl = nullptr;  // pinned host
  bpsr::BlockqCtl* hctl_dev = nullptr;
  uint32_t* kcnt = nullptr;         // device, one tile counter per block
  uint32_t* khdone = nullptr;       // pinned host, one completion word per block
  uint32_t* khdone_dev = nullptr;
  uint32_t opened = 0;              // highest epoch a round was released for (keyq_opened)
  int last_pol = bpsr::kPolPlain;   // cache policy of the latest keyq_launch (keyq_shape)
#ifdef BPSR_KEYED_TRACE
  unsigned long long* ktrace = nullptr;  // probe builds: kKtraceSlots launches' stamps
  size_t ktrace_per = 0;
#endif
};

namespace bpsr {

constexpr uint32_t kKtraceSlots = 64;  // probe builds (BPSR_KEYED_TRACE)

// q->mu held.  What every launch of `epoch` carries — table, release words,
// control word, timeout, epoch; everything else null or 0 — and its cache
// policy under `tu`.
BlockqLaunch blockq_launch_args(const byteps_reduce_blockq* q, uint32_t epoch, const Tuning& tu,
                                int* pol);

}  // namespace bpsr
