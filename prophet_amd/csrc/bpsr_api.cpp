// C ABI of libbpsr.so (include/bpsr/reduce.h): errors, tuning, descriptor
// staging and the fold, batched, plan, copy and cast calls.  The batch tables
// are bpsr_table.cpp, the block queue bpsr_blockq.cpp (on bpsr_queues.cpp),
// the keyed queue bpsr_keyq.cpp.  Never aborts: every failure is a negative
// status plus a thread-local message.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "bpsr_api_internal.h"

namespace bpsr {

static thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_last_error = buf;
  return code;
}

int hip_fail(hipError_t e, const char* what) {
  return fail(BYTEPS_REDUCE_EHIP, "%s: %s", what, hipGetErrorString(e));
}

// Process-wide tuning, read by every launch (engine lanes and caller threads)
// and written by byteps_reduce_set_tuning: launches take a snapshot under the
// lock, so a concurrent set_tuning never tears a launch's geometry.
static std::mutex g_tuning_mu;
thread_local int t_occ_floor = 0;
thread_local std::atomic<const char*>* t_where = nullptr;

static Tuning& tuning_storage() {
  static Tuning tu = [] {
    // tools/sweep.py, tools/occ_sweep.py, tools/cfg3_probe.py (profiles/)
    Tuning t{2, 1, 1 << 20, 1, 2, 0, 4096, 4096, 1, 4, 2, kWtMaxBytes};
    if (const char* v = getenv("BPSR_WT_MAX_MIB")) t.wt_max_bytes = (uint64_t)atoll(v) << 20;
    if (const char* v = getenv("BPSR_COPY_OCC")) t.copy_occ = atoi(v);
    if (const char* v = getenv("BPSR_COPY_VPT")) t.copy_vpt = atoi(v);
    if (t.copy_occ < 0 || t.copy_occ > 8) t.copy_occ = 4;
    if (t.copy_vpt != 1 && t.copy_vpt != 4) t.copy_vpt = 2;
    if (const char* v = getenv("BPSR_OCC_MIN_TILES")) t.occ_min_tiles = (uint32_t)atol(v);
    if (const char* v = getenv("BPSR_OCC_MIN_TILES_BATCH"))
      t.occ_min_tiles_batch = (uint32_t)atol(v);
    if (const char* v = getenv("BPSR_AUTO_N")) t.auto_n = atoi(v) != 0;
    if (const char* v = getenv("BPSR_VPT")) t.vpt = atoi(v);
    if (const char* v = getenv("BPSR_NT")) t.nt = atoi(v);
    if (const char* v = getenv("BPSR_MAX_GRID")) t.max_grid = atoi(v);
    if (const char* v = getenv("BPSR_OCC")) t.occ = atoi(v);
    if (const char* v = getenv("BPSR_SMALL_OCC")) t.small_occ = atoi(v);
    if (const char* v = getenv("BPSR_SMALL_OCC_BATCH")) t.small_occ_batch = atoi(v);
    if (t.small_occ < 0 || t.small_occ > 8) t.small_occ = 2;
    if (t.small_occ_batch < 0 || t.small_occ_batch > 8) t.small_occ_batch = 0;
    if (t.vpt != 1 && t.vpt != 4) t.vpt = 2;
    if (t.occ < 0 || t.occ > 8) t.occ = 1;
    if (t.max_grid < 1) t.max_grid = 1 << 20;
    t.nt = t.nt ? 1 : 0;
    return t;
  }();
  return tu;
}

static Tuning tuning() {
  std::lock_guard<std::mutex> g(g_tuning_mu);
  return tuning_storage();
}

// Bytes in flight per CU = residency x 256 lanes x n sources x vpt x 16 B.
// The defaults (1 workgroup per CU, vpt 2) give 64 KiB at the 8-way fold;
// with n <= 4 sources that leaves the HBM queues short, and 2 workgroups per
// CU with 16 KiB tiles measured +13-26 % (profiles/r01_nsweep.jsonl: 2-way
// 256 MiB 5.21 -> 6.56 TB/s).  Applies unless BPSR_AUTO_N=0.
static Tuning tuning_for_n(int n) {
  Tuning t = tuning();
  if (t.auto_n && n <= 4 && t.occ == 1) {
    t.occ = 2;
    t.vpt = 4;
  }
  return t;
}

static inline hipStream_t to_stream(void* s) { return stream_of(s); }

// The tuning as the other units of the ABI see it (bpsr_api_internal.h).
Tuning launch_tuning_for_n(int n) { return tuning_for_n(n); }

// One fold launch over at most kMaxSrcs sources.
static int fold_once(void* dst, const void* const* srcs, int n, size_t len, int dtype,
                     int mode, bool copy_trailing, hipStream_t s) {
  FoldArgs a;
  std::memset(&a, 0, sizeof(a));
  for (int k = 0; k < n; ++k) a.srcs[k] = static_cast<const unsigned char*>(srcs[k]);
  a.dst = static_cast<unsigned char*>(dst);
  a.n = n;
  make_geom(dtype, len, dst, srcs, n, copy_trailing, &a.g, &a.aligned);
  hipError_t e = launch_fold(a, dtype, mode, tuning_for_n(n), s);
  if (e != hipSuccess) return hip_fail(e, "fold kernel launch");
  return BYTEPS_REDUCE_OK;
}

// ------------------------------------------------ batched descriptor staging --
// Per-thread ring of pinned host + device tables.  A slot is reused only after
// the event recorded behind the kernel that read it has completed.
struct StageSlot {
  int device = -1;
  size_t cap = 0;
  void* host = nullptr;      // pinned, coherent (the device reads it uncached)
  void* host_dev = nullptr;  // the same pages as the device addresses them
  void* dev = nullptr;
  hipEvent_t done = nullptr;
  bool pending = false;
};
constexpr int kRing = 8;
// Tables up to this size are read by the kernel straight from the pinned
// staging slot (each workgroup fetches its own record over PCIe once) instead
// of being copied to HBM first: a small hipMemcpyAsync H2D waits for the
// stream's earlier work on the host (130-380 us per call behind queued folds,
// rocprofv3 HIP trace of the server's issuer threads).
constexpr size_t kZeroCopyTable = 256 * 1024;  // default; a ring may read larger ones in place

struct StageRing {
  StageSlot slots[kRing];
  int next = 0;
  size_t zero_copy_max = kZeroCopyTable;
  std::vector<char> table;  // host copy of the table being built
  // Buffers a slot outgrew: freed with the ring, never while it is in use —
  // hipFree waits for the whole device, and a server lane's issuer must not
  // wait for a running keyed consumer that waits for the releases it queues.
  std::vector<void*> retired_host, retired_dev;
  ~StageRing() {
    for (auto& s : slots) {
      if (s.pending && s.done) (void)hipEventSynchronize(s.done);
      if (s.done) (void)hipEventDestroy(s.done);
      if (s.host) (void)hipHostFree(s.host);
      if (s.dev) (void)hipFree(s.dev);
    }
    for (void* p : retired_host) (void)hipHostFree(p);
    for (void* p : retired_dev) (void)hipFree(p);
  }
};
static thread_local StageRing g_ring;

StageRing* stage_ring_create(size_t zero_copy_max) {
  auto* r = new StageRing();
  if (zero_copy_max) r->zero_copy_max = zero_copy_max;
  return r;
}
void stage_ring_destroy(StageRing* r) { delete r; }

static int stage_acquire(StageRing& ring, size_t bytes, StageSlot** out) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
  StageSlot& s = ring.slots[ring.next];
  ring.next = (ring.next + 1) % kRing;
  if (s.pending) {
    note_where("ring: slot event sync");
    e = hipEventSynchronize(s.done);
    if (e != hipSuccess) return hip_fail(e, "hipEventSynchronize(stage)");
    s.pending = false;
  }
  if (s.device != dev || s.cap < bytes) {
    // the outgrown buffers are retired, not freed (see StageRing)
    if (s.host) ring.retired_host.push_back(s.host);
    if (s.dev) ring.retired_dev.push_back(s.dev);
    if (s.done) (void)hipEventDestroy(s.done);
    s.host = s.host_dev = s.dev = nullptr;
    s.done = nullptr;
    note_where("ring: grow");
    // grow geometrically: freeing pinned memory synchronises the device
    const size_t cap = std::max<size_t>({bytes, 2 * s.cap, kZeroCopyTable});
    s.cap = 0;
    if ((e = hipHostMalloc(&s.host, cap, hipHostMallocMapped | hipHostMallocCoherent)) !=
        hipSuccess)
      return hip_fail(e, "hipHostMalloc(stage)");
    if ((e = hipHostGetDevicePointer(&s.host_dev, s.host, 0)) != hipSuccess)
      return hip_fail(e, "hipHostGetDevicePointer(stage)");
    if ((e = hipMalloc(&s.dev, cap)) != hipSuccess) return hip_fail(e, "hipMalloc(stage)");
    if ((e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming)) != hipSuccess)
      return hip_fail(e, "hipEventCreate(stage)");
    s.cap = cap;
    s.device = dev;
  }
  *out = &s;
  return BYTEPS_REDUCE_OK;
}


int batched_with_ring(const byteps_bucket_desc* buckets, int nbuckets, int dtype, int mode,
                      hipStream_t s, StageRing* ring, hipEvent_t* done) {
  if (done) *done = nullptr;
  int rc = check_common(dtype, mode);
  if (rc) return rc;
  if (nbuckets < 0 || (nbuckets > 0 && !buckets))
    return fail(BYTEPS_REDUCE_EARGS, "bad bucket table");
  if (nbuckets == 0) return BYTEPS_REDUCE_OK;
  TableInfo ti;
  if ((rc = build_table(buckets, nbuckets, dtype, ring->table, &ti))) return rc;
  if (ti.tiles == 0) return BYTEPS_REDUCE_OK;
  StageSlot* slot = nullptr;
  if ((rc = stage_acquire(*ring, ti.bytes, &slot))) return rc;
  std::memcpy(slot->host, ring->table.data(), ti.bytes);
  hipError_t e = hipSuccess;
  const void* table = slot->host_dev;
  note_where("ring: table copy");
  if (ti.bytes > ring->zero_copy_max) {  // large: one H2D copy, the kernel reads HBM
    e = hipMemcpyAsync(slot->dev, slot->host, ti.bytes, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(batch table)");
    table = slot->dev;
  }
  // (The slot's event stays a separate record: completing it by the launch
  // itself, like the block queue's join, made the server's lane issuers see
  // completions sooner and split config 3's rounds into more, smaller
  // launches — 33-43 instead of 23-31 per round at 4 lanes, r03s57.)
  note_where("ring: kernel launch");
  e = launch_batched(batch_launch(table, ti, table == slot->dev), ti.vpt, dtype, mode,
                     tuning_for_n(ti.nmax), s);
  note_where("ring: event record");
  if (e != hipSuccess) return hip_fail(e, "batched kernel launch");
  e = hipEventRecord(slot->done, s);
  if (e != hipSuccess) return hip_fail(e, "hipEventRecord(stage)");
  slot->pending = true;
  if (done) *done = slot->done;
  return BYTEPS_REDUCE_OK;
}

int fold_alias_check(const void* dst, const void* const* srcs, int n, size_t len) {
  if (n < 1 || !srcs) return fail(BYTEPS_REDUCE_EARGS, "need n >= 1 sources (n=%d)", n);
  if (len == 0) return BYTEPS_REDUCE_OK;
  if (!dst) return fail(BYTEPS_REDUCE_EARGS, "null dst");
  int alias = -1;
  for (int k = 0; k < n; ++k) {
    if (!srcs[k]) return fail(BYTEPS_REDUCE_EARGS, "null srcs[%d]", k);
    if (overlaps_partially(dst, srcs[k], len))
      return fail(BYTEPS_REDUCE_EARGS, "dst partially overlaps srcs[%d]", k);
    if (srcs[k] != dst) continue;
    if (alias >= 0) return fail(BYTEPS_REDUCE_EARGS, "dst aliases two sources");
    alias = k;
  }
  if (alias > 0 && n > kMaxSrcs)
    return fail(BYTEPS_REDUCE_EARGS, "dst aliases srcs[%d] of a %d-way fold (> %d)", alias, n,
                kMaxSrcs);
  return BYTEPS_REDUCE_OK;
}

int fold_any_alias(void* dst, const void* const* srcs, int n, size_t len, int dtype, int mode,
                   hipStream_t s) {
  int rc = check_common(dtype, mode);
  if (rc) return rc;
  if ((rc = fold_alias_check(dst, srcs, n, len))) return rc;
  int alias = -1;
  for (int k = 0; k < n; ++k)
    if (srcs[k] == dst) alias = k;
  if (alias <= 0) return byteps_reduce_sum_n(dst, srcs, n, len, dtype, mode, s);
  if (len == 0) return BYTEPS_REDUCE_OK;
  return fold_once(dst, srcs, n, len, dtype, mode, /*copy_trailing=*/true, s);
}

}  // namespace bpsr

using namespace bpsr;

extern "C" {

int byteps_reduce_version(void) { return BYTEPS_REDUCE_ABI_VERSION; }

int byteps_reduce_dtype_size(int dtype) {
  const int es = elem_size(dtype);
  return es ? es : fail(BYTEPS_REDUCE_EDTYPE, "Unsupported data type: %d", dtype);
}

const char* byteps_reduce_last_error(void) { return g_last_error.c_str(); }

int byteps_reduce_set_tuning(int vpt, int nt, int max_grid, int occ) {
  // validate everything before changing anything
  if (vpt > 0 && vpt != 1 && vpt != 2 && vpt != 4)
    return fail(BYTEPS_REDUCE_EARGS, "vpt must be 1, 2 or 4");
  if (occ > 8) return fail(BYTEPS_REDUCE_EARGS, "occ must be 0..8");
  std::lock_guard<std::mutex> g(g_tuning_mu);
  Tuning& t = tuning_storage();
  if (vpt > 0) t.vpt = vpt;
  if (nt >= 0) t.nt = nt ? 1 : 0;
  if (max_grid > 0) t.max_grid = max_grid;
  if (occ >= 0) t.occ = occ;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_get_tuning(int* vpt, int* nt, int* max_grid, int* occ) {
  const Tuning t = tuning();
  if (vpt) *vpt = t.vpt;
  if (nt) *nt = t.nt;
  if (max_grid) *max_grid = t.max_grid;
  if (occ) *occ = t.occ;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_init(int device) {
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
  (void)tuning();
  e = hipFree(nullptr);  // forces context creation
  if (e != hipSuccess) return hip_fail(e, "hip runtime init");
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_shutdown(void) {
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return hip_fail(e, "hipDeviceSynchronize");
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_sum(void* dst, const void* src, size_t len, int dtype, void* stream) {
  int rc = check_common(dtype, kModeReference);
  if (rc) return rc;
  if (len == 0) return BYTEPS_REDUCE_OK;
  if (!dst || !src) return fail(BYTEPS_REDUCE_EARGS, "null pointer");
  if (overlaps_partially(dst, src, len))
    return fail(BYTEPS_REDUCE_EARGS, "dst and src partially overlap");
  const void* srcs[2] = {dst, src};
  return fold_once(dst, srcs, 2, len, dtype, kModeReference, false, to_stream(stream));
}

int byteps_reduce_sum3(void* dst, const void* src1, const void* src2, size_t len, int dtype,
                       void* stream) {
  int rc = check_common(dtype, kModeReference);
  if (rc) return rc;
  if (len == 0) return BYTEPS_REDUCE_OK;
  if (!dst || !src1 || !src2) return fail(BYTEPS_REDUCE_EARGS, "null pointer");
  if (overlaps_partially(dst, src1, len) || overlaps_partially(dst, src2, len))
    return fail(BYTEPS_REDUCE_EARGS, "dst partially overlaps a source");
  // fp16: the reference's compiled 3-operand body keeps src2's NaN when both
  // operands are NaN (the in-place body keeps dst's), so src2 is folded first;
  // nothing else in the add depends on the operands' order.
  const bool swap = dtype == BYTEPS_REDUCE_FLOAT16;
  const void* srcs[2] = {swap ? src2 : src1, swap ? src1 : src2};
  return fold_once(dst, srcs, 2, len, dtype, kModeReference, false, to_stream(stream));
}

int byteps_reduce_sum_n(void* dst, const void* const* srcs, int n, size_t len, int dtype,
                        int mode, void* stream) {
  int rc = check_common(dtype, mode);
  if (rc) return rc;
  if (n < 1 || !srcs) return fail(BYTEPS_REDUCE_EARGS, "need n >= 1 sources (n=%d)", n);
  if (len == 0) return BYTEPS_REDUCE_OK;
  if (!dst) return fail(BYTEPS_REDUCE_EARGS, "null dst");
  for (int k = 0; k < n; ++k) {
    if (!srcs[k]) return fail(BYTEPS_REDUCE_EARGS, "null srcs[%d]", k);
    if (overlaps_partially(dst, srcs[k], len))
      return fail(BYTEPS_REDUCE_EARGS, "dst partially overlaps srcs[%d]", k);
    if (k > 0 && srcs[k] == dst)
      return fail(BYTEPS_REDUCE_EARGS, "dst may alias only srcs[0] (srcs[%d] == dst)", k);
  }
  hipStream_t s = to_stream(stream);
  if (n == 1) {
    if (dst == srcs[0]) return BYTEPS_REDUCE_OK;
    hipError_t e = launch_copy(dst, srcs[0], len, tuning(), s);
    return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "copy kernel launch");
  }
  // First launch folds up to kMaxSrcs sources; each further launch folds the
  // running result (as its srcs[0]) with the next kMaxSrcs-1: still a strict
  // left fold, bit-exact in reference mode.
  int take = std::min(n, kMaxSrcs);
  rc = fold_once(dst, srcs, take, len, dtype, mode, dst != srcs[0], s);
  const void* chunk[kMaxSrcs];
  for (int k = take; rc == 0 && k < n;) {
    int m = std::min(n - k, kMaxSrcs - 1);
    chunk[0] = dst;
    for (int j = 0; j < m; ++j) chunk[1 + j] = srcs[k + j];
    rc = fold_once(dst, chunk, m + 1, len, dtype, mode, false, s);
    k += m;
  }
  return rc;
}

int byteps_reduce_sum_batched(const byteps_bucket_desc* buckets, int nbuckets, int dtype,
                              int mode, void* stream) {
  // the calling thread's staging ring (pinned table + device copy, reused
  // once the kernel that read a slot has completed)
  return batched_with_ring(buckets, nbuckets, dtype, mode, to_stream(stream), &g_ring);
}

struct byteps_reduce_plan {
  int device;
  int dtype;
  int mode;
  void* dev_table;
  TableInfo ti;
};

int byteps_reduce_plan_create(const byteps_bucket_desc* buckets, int nbuckets, int dtype,
                              int mode, byteps_reduce_plan** out) {
  if (!out) return fail(BYTEPS_REDUCE_EARGS, "null plan out-pointer");
  *out = nullptr;
  int rc = check_common(dtype, mode);
  if (rc) return rc;
  if (nbuckets < 0 || (nbuckets > 0 && !buckets))
    return fail(BYTEPS_REDUCE_EARGS, "bad bucket table");
  std::vector<char> host;
  TableInfo ti;
  if ((rc = build_table(buckets, nbuckets, dtype, host, &ti))) return rc;
  auto* p = new byteps_reduce_plan();
  p->dtype = dtype;
  p->mode = mode;
  p->ti = ti;
  p->dev_table = nullptr;
  hipError_t e = hipGetDevice(&p->device);
  if (e == hipSuccess && ti.tiles > 0) {
    e = hipMalloc(&p->dev_table, ti.bytes);
    if (e == hipSuccess)
      e = hipMemcpy(p->dev_table, host.data(), ti.bytes, hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    if (p->dev_table) (void)hipFree(p->dev_table);
    delete p;
    return hip_fail(e, "plan table upload");
  }
  *out = p;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_plan_launch(byteps_reduce_plan* p, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (p->ti.tiles == 0) return BYTEPS_REDUCE_OK;
  hipError_t e = launch_batched(batch_launch(p->dev_table, p->ti), p->ti.vpt, p->dtype, p->mode,
                                tuning_for_n(p->ti.nmax), to_stream(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "plan kernel launch");
}

int byteps_reduce_plan_destroy(byteps_reduce_plan* p) {
  if (!p) return BYTEPS_REDUCE_OK;
  hipError_t e = hipSuccess;
  if (p->dev_table) e = hipFree(p->dev_table);
  delete p;
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "plan free");
}

int byteps_reduce_copy(void* dst, const void* src, size_t len, void* stream) {
  if (len == 0 || dst == src) return BYTEPS_REDUCE_OK;
  if (!dst || !src) return fail(BYTEPS_REDUCE_EARGS, "null pointer");
  if (overlaps_partially(dst, src, len))
    return fail(BYTEPS_REDUCE_EARGS, "dst and src overlap");
  hipError_t e = launch_copy(dst, src, len, tuning(), to_stream(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "copy kernel launch");
}

}  // extern "C"

// ------------------------------------------------------------------ casts --
// The launch wrappers of one wire format (bpsr_internal.h): the single casts,
// and the plan's per direction and scheme.
struct CastWire {
  int wire;
  decltype(launch_compress_fp16)* compress;
  decltype(launch_decompress_fp16)* decompress;
  decltype(launch_compress_ef)* compress_ef;
  decltype(launch_compress_sr)* compress_sr;
  decltype(launch_cast_plan)* plan;
  decltype(launch_cast_plan_ef)* plan_ef;
  decltype(launch_cast_plan_sr)* plan_sr;
  decltype(launch_cast_plan_stats)* plan_stats;
  decltype(launch_cast_plan_measure)* plan_measure;
  decltype(launch_cast_plan_scaled)* plan_scaled;
  decltype(launch_cast_plan_sgd)* plan_sgd;
};
static const CastWire kCastWires[] = {
    {kFloat16, launch_compress_fp16, launch_decompress_fp16, launch_compress_ef,
     launch_compress_sr, launch_cast_plan, launch_cast_plan_ef, launch_cast_plan_sr,
     launch_cast_plan_stats, launch_cast_plan_measure, launch_cast_plan_scaled,
     launch_cast_plan_sgd},
    {kBFloat16, launch_compress_bf16, launch_decompress_bf16, launch_compress_ef_bf16,
     launch_compress_sr_bf16, launch_cast_plan_bf16, launch_cast_plan_ef_bf16,
     launch_cast_plan_sr_bf16, launch_cast_plan_stats_bf16, launch_cast_plan_measure_bf16,
     launch_cast_plan_scaled_bf16, launch_cast_plan_sgd_bf16},
};

// The row of a wire format; null, with the dtype error set, for any other.
static const CastWire* cast_wire(int wire) {
  for (const CastWire& w : kCastWires)
    if (w.wire == wire) return &w;
  fail(BYTEPS_REDUCE_EDTYPE, "compression to data type %d", wire);
  return nullptr;
}

// A single cast: every check before any HIP call (cast_check), then `launch`
// with the wire's row; `what` names the launch in a HIP error.
template <class Launch>
static int cast_single(int wire, int wide_dtype, CastScheme scheme, int divisor, size_t nelem,
                       std::initializer_list<CastOperand> ops, const char* what, Launch launch) {
  const int rc =
      cast_check(wire, wide_dtype, scheme, divisor, nelem, ops.begin(), (int)ops.size());
  if (rc != BYTEPS_REDUCE_OK) return rc > 0 ? BYTEPS_REDUCE_OK : rc;
  const hipError_t e = launch(*cast_wire(wire));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, what);
}

struct byteps_reduce_cast_plan {
  int device;
  int dtype;
  const CastWire* wire;
  CastScheme scheme;  // also for a plan without records
  CastTableInfo ti;
  int nsegs;
  // What the plan owns on the device: the table; for the decompress statistics
  // (_decompress_stats) the segments' record lists, seg_begin[nsegs + 1] then
  // seg_recs[records], uploaded with the table, and the (record, wave)
  // partials, made by the first statistics call; and the scheme's array of one
  // entry per record — a residual pointer (error feedback), a CastSrRec
  // (stochastic rounding) or a momentum pointer (an SGD plan, whose wide side
  // is the parameter).
  enum { kTable, kSeg, kPart, kSide, kDevArrays };
  void* dev[kDevArrays] = {};
  // the segments' byte ranges, which the statistics' output must stay clear of
  std::vector<std::pair<uintptr_t, uintptr_t>> ranges;
};

// Frees what the plan owns and the plan; the first error wins.
static hipError_t cast_plan_free(byteps_reduce_cast_plan* p) {
  hipError_t e = hipSuccess;
  for (void* q : p->dev)
    if (q) {
      const hipError_t e2 = hipFree(q);
      if (e == hipSuccess) e = e2;
    }
  delete p;
  return e;
}

// A host array as a new device array.
template <class T>
static hipError_t cast_plan_upload(void** dev, const std::vector<T>& host) {
  const size_t bytes = host.size() * sizeof(T);
  const hipError_t e = hipMalloc(dev, bytes);
  return e == hipSuccess ? hipMemcpy(*dev, host.data(), bytes, hipMemcpyHostToDevice) : e;
}

// The three table builders under one name: `side` is the scheme's array of one
// entry per record (none for a plain plan).
static int cast_plan_table(const byteps_cast_desc* segs, int nsegs, int dtype, int copy_vpt,
                           std::vector<char>& out, std::vector<char>& /*side*/, CastTableInfo* ti,
                           CastSegList* lists) {
  return build_cast_table(segs, nsegs, dtype, copy_vpt, out, ti, lists);
}
static int cast_plan_table(const byteps_cast_ef_desc* segs, int nsegs, int dtype, int copy_vpt,
                           std::vector<char>& out, std::vector<unsigned char*>& side,
                           CastTableInfo* ti, CastSegList* lists) {
  return build_cast_table_ef(segs, nsegs, dtype, copy_vpt, out, side, ti, lists);
}
static int cast_plan_table(const byteps_cast_sr_desc* segs, int nsegs, int dtype, int copy_vpt,
                           std::vector<char>& out, std::vector<CastSrRec>& side, CastTableInfo* ti,
                           CastSegList* lists) {
  return build_cast_table_sr(segs, nsegs, dtype, copy_vpt, out, side, ti, lists);
}

// An SGD plan's table is an error-feedback plan's, unchanged: wide = the
// parameter, resid = the momentum buffer (cast_cut_ef's co-alignment rule, the
// 3 * nsegs disjoint ranges and the parallel pointer array are what it needs).
static int cast_plan_table(const byteps_cast_sgd_desc* segs, int nsegs, int dtype, int copy_vpt,
                           std::vector<char>& out, std::vector<unsigned char*>& side,
                           CastTableInfo* ti, CastSegList* lists) {
  if (nsegs < 0 || (nsegs > 0 && !segs)) return fail(BYTEPS_REDUCE_EARGS, "bad segment table");
  std::vector<byteps_cast_ef_desc> ef((size_t)nsegs);
  for (int i = 0; i < nsegs; ++i)
    ef[(size_t)i] = byteps_cast_ef_desc{segs[i].param, segs[i].half, segs[i].momentum,
                                        segs[i].nelem};
  return build_cast_table_ef(ef.data(), nsegs, dtype, copy_vpt, out, side, ti, lists);
}

// A new plan of `scheme`: build the table (and the scheme's array, of `Side`
// entries), take the byte ranges the builder tested, and upload — the record
// lists whenever the plan has a segment, records or not.
template <class Side, class D>
static int cast_plan_create(CastScheme scheme, const D* segs, int nsegs, int wide_dtype, int wire,
                            byteps_reduce_cast_plan** out) {
  if (!out) return fail(BYTEPS_REDUCE_EARGS, "null plan out-pointer");
  *out = nullptr;
  const int pair = cast_dtype_check(wire, wide_dtype, scheme);
  if (pair != BYTEPS_REDUCE_OK) return pair;
  // The table builder cuts by element size alone and knows the fp16 wire's
  // three wide types, so a wide fp16 (bf16 wire) is cut as its 2-byte peer.
  const int table_dtype = wide_dtype == kFloat16 ? kBFloat16 : wide_dtype;
  std::vector<char> host;
  std::vector<Side> side;
  CastTableInfo ti;
  CastSegList lists;
  const int rc =
      cast_plan_table(segs, nsegs, table_dtype, tuning().copy_vpt, host, side, &ti, &lists);
  if (rc) return rc;
  auto* p = new byteps_reduce_cast_plan();
  p->dtype = wide_dtype;
  p->wire = cast_wire(wire);
  p->scheme = scheme;
  p->ti = ti;
  p->nsegs = nsegs;
  p->ranges = std::move(lists.ranges);
  hipError_t e = hipGetDevice(&p->device);
  if (e == hipSuccess && nsegs > 0) {
    std::vector<uint32_t>& seg = lists.seg_begin;
    seg.insert(seg.end(), lists.seg_recs.begin(), lists.seg_recs.end());
    e = cast_plan_upload(&p->dev[p->kSeg], seg);
  }
  if (e == hipSuccess && ti.records > 0) {
    e = cast_plan_upload(&p->dev[p->kTable], host);
    if (e == hipSuccess && scheme != kCastPlain) e = cast_plan_upload(&p->dev[p->kSide], side);
  }
  if (e != hipSuccess) {
    (void)cast_plan_free(p);
    return hip_fail(e, "cast plan table upload");
  }
  *out = p;
  return BYTEPS_REDUCE_OK;
}

// Every plan call but _apply_sgd and _destroy refuses an SGD plan: its wide
// side is the parameter, which a decompress would overwrite with gradients.
static int refuse_sgd(const byteps_reduce_cast_plan* p, const char* what) {
  if (p->scheme != kCastSgd) return BYTEPS_REDUCE_OK;
  return fail(BYTEPS_REDUCE_EARGS,
              "%s on an SGD plan: its wide side is the parameter "
              "(byteps_reduce_cast_plan_apply_sgd)", what);
}

// The plan's one launch, by direction and scheme (validated by the callers;
// the plan has records): a compress is its scheme's — `step` for stochastic
// rounding — a decompress the plain one for every scheme, with the statistics'
// partials where `part` is not null — without the stores where `measure` is
// set — and times *mult where `mult` is not null.
static int cast_plan_launch(byteps_reduce_cast_plan* p, bool compress, int divisor, uint32_t step,
                            void* part, void* stream, bool measure = false,
                            const float* mult = nullptr) {
  const CastRec* table = static_cast<const CastRec*>(p->dev[p->kTable]);
  void* side = p->dev[p->kSide];
  const uint32_t n = p->ti.records;
  const int u = p->ti.u;
  const uint64_t wide_bytes = p->ti.nelem * (uint64_t)elem_size(p->dtype);
  const Tuning tu = tuning();
  hipStream_t s = to_stream(stream);
  hipError_t e;
  if (!compress && mult)
    e = p->wire->plan_scaled(table, n, p->dtype, divisor, u, wide_bytes, mult, tu, s);
  else if (!compress && measure)
    e = p->wire->plan_measure(table, n, p->dtype, divisor, u, part, tu, s);
  else if (!compress)
    e = part ? p->wire->plan_stats(table, n, p->dtype, divisor, u, wide_bytes, part, tu, s)
             : p->wire->plan(false, table, n, p->dtype, divisor, u, wide_bytes, tu, s);
  else if (p->scheme == kCastEf)  // 2 + 4 bytes written an element
    e = p->wire->plan_ef(table, static_cast<unsigned char* const*>(side), n, u, p->ti.nelem * 6,
                         tu, s);
  else if (p->scheme == kCastSr)
    e = p->wire->plan_sr(table, static_cast<const CastSrRec*>(side), n, step, u, p->ti.nelem * 2,
                         tu, s);
  else
    e = p->wire->plan(true, table, n, p->dtype, 1, u, p->ti.nelem * 2, tu, s);
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "cast plan kernel launch");
}

extern "C" {

int byteps_reduce_compress_to(void* dst, const void* src, size_t nelem, int src_dtype,
                              int wire_dtype, void* stream) {
  return cast_single(wire_dtype, src_dtype, kCastPlain, 1, nelem,
                     {{"dst", dst, 2}, {"src", src, (size_t)elem_size(src_dtype)}},
                     "compress kernel launch", [&](const CastWire& w) {
                       return w.compress(dst, src, nelem, src_dtype, tuning(), to_stream(stream));
                     });
}

int byteps_reduce_decompress_from(void* dst, const void* src, size_t nelem, int dst_dtype,
                                  int wire_dtype, int divisor, void* stream) {
  return cast_single(wire_dtype, dst_dtype, kCastPlain, divisor, nelem,
                     {{"dst", dst, (size_t)elem_size(dst_dtype)}, {"src", src, 2}},
                     "decompress kernel launch", [&](const CastWire& w) {
                       return w.decompress(dst, src, nelem, dst_dtype, divisor, tuning(),
                                           to_stream(stream));
                     });
}

int byteps_reduce_compress_fp16(void* dst, const void* src, size_t nelem, int src_dtype,
                                void* stream) {
  return byteps_reduce_compress_to(dst, src, nelem, src_dtype, kFloat16, stream);
}

int byteps_reduce_decompress_fp16(void* dst, const void* src, size_t nelem, int dst_dtype,
                                  int divisor, void* stream) {
  return byteps_reduce_decompress_from(dst, src, nelem, dst_dtype, kFloat16, divisor, stream);
}

// dst and resid are written, src is read: three pairwise disjoint ranges.
int byteps_reduce_compress_ef(void* dst, void* resid, const void* src, size_t nelem,
                              int src_dtype, int wire_dtype, void* stream) {
  return cast_single(wire_dtype, src_dtype, kCastEf, 1, nelem,
                     {{"dst", dst, 2}, {"resid", resid, 4}, {"src", src, 4}},
                     "error-feedback compress kernel launch", [&](const CastWire& w) {
                       return w.compress_ef(dst, resid, src, nelem, tuning(), to_stream(stream));
                     });
}

int byteps_reduce_compress_sr(void* dst, const void* src, size_t nelem, int src_dtype,
                              int wire_dtype, uint32_t key, uint32_t step, void* stream) {
  return cast_single(wire_dtype, src_dtype, kCastSr, 1, nelem, {{"dst", dst, 2}, {"src", src, 4}},
                     "stochastic-rounding compress kernel launch", [&](const CastWire& w) {
                       return w.compress_sr(dst, src, nelem, key, step, tuning(),
                                            to_stream(stream));
                     });
}

int byteps_reduce_cast_plan_create_wire(const byteps_cast_desc* segs, int nsegs, int wide_dtype,
                                        int wire_dtype, byteps_reduce_cast_plan** out) {
  return cast_plan_create<char>(kCastPlain, segs, nsegs, wide_dtype, wire_dtype, out);
}

int byteps_reduce_cast_plan_create(const byteps_cast_desc* segs, int nsegs, int wide_dtype,
                                   byteps_reduce_cast_plan** out) {
  return byteps_reduce_cast_plan_create_wire(segs, nsegs, wide_dtype, kFloat16, out);
}

int byteps_reduce_cast_plan_create_ef(const byteps_cast_ef_desc* segs, int nsegs, int wide_dtype,
                                      int wire_dtype, byteps_reduce_cast_plan** out) {
  return cast_plan_create<unsigned char*>(kCastEf, segs, nsegs, wide_dtype, wire_dtype, out);
}

int byteps_reduce_cast_plan_create_sr(const byteps_cast_sr_desc* segs, int nsegs, int wide_dtype,
                                      int wire_dtype, byteps_reduce_cast_plan** out) {
  return cast_plan_create<CastSrRec>(kCastSr, segs, nsegs, wide_dtype, wire_dtype, out);
}

int byteps_reduce_cast_plan_compress(byteps_reduce_cast_plan* p, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (const int rc = refuse_sgd(p, "compress")) return rc;
  if (p->scheme == kCastSr)
    return fail(BYTEPS_REDUCE_EARGS,
                "a stochastic-rounding plan is compressed with a step "
                "(byteps_reduce_cast_plan_compress_sr)");
  if (p->ti.records == 0) return BYTEPS_REDUCE_OK;
  return cast_plan_launch(p, true, 1, 0, nullptr, stream);
}

int byteps_reduce_cast_plan_compress_sr(byteps_reduce_cast_plan* p, uint32_t step, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (const int rc = refuse_sgd(p, "compress_sr")) return rc;
  if (p->scheme != kCastSr)
    return fail(BYTEPS_REDUCE_EARGS, "the plan carries no keys (byteps_reduce_cast_plan_create_sr)");
  if (p->ti.records == 0) return BYTEPS_REDUCE_OK;
  return cast_plan_launch(p, true, 1, step, nullptr, stream);
}

int byteps_reduce_cast_plan_decompress(byteps_reduce_cast_plan* p, int divisor, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (const int rc = refuse_sgd(p, "decompress")) return rc;
  if (divisor < 1) return fail(BYTEPS_REDUCE_EARGS, "divisor %d < 1", divisor);
  if (p->ti.records == 0) return BYTEPS_REDUCE_OK;
  return cast_plan_launch(p, false, divisor, 0, nullptr, stream);
}

// _decompress_stats and _measure: the checks, the partials, the decompress
// with or without its stores, the finish.
static int cast_plan_stats(byteps_reduce_cast_plan* p, int divisor, double* stats, void* stream,
                           bool measure) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (const int rc = refuse_sgd(p, measure ? "measure" : "decompress_stats")) return rc;
  if (divisor < 1) return fail(BYTEPS_REDUCE_EARGS, "divisor %d < 1", divisor);
  if (p->nsegs <= 0) return BYTEPS_REDUCE_OK;  // no segment: no row, nothing to write
  if (!stats) return fail(BYTEPS_REDUCE_EARGS, "null stats pointer");
  const uintptr_t sb = (uintptr_t)stats;
  const size_t bytes = (size_t)p->nsegs * 2 * sizeof(double);
  if (sb % sizeof(double)) return fail(BYTEPS_REDUCE_EARGS, "stats is not 8-byte aligned");
  if (sb > UINTPTR_MAX - bytes)
    return fail(BYTEPS_REDUCE_EARGS, "stats wraps the address space");
  for (const auto& r : p->ranges)
    if (sb < r.second && r.first < sb + bytes)
      return fail(BYTEPS_REDUCE_EARGS, "stats overlaps a segment of the plan");
  void*& part = p->dev[p->kPart];
  if (p->ti.records > 0) {
    if (!part) {  // the first statistics call of a plan allocates
      hipError_t e = hipMalloc(&part, (size_t)p->ti.records * kStatPartBytes);
      if (e != hipSuccess) return hip_fail(e, "cast plan statistics partials");
    }
    const int rc = cast_plan_launch(p, false, divisor, 0, part, stream, measure);
    if (rc) return rc;
  }
  const uint32_t* seg = static_cast<const uint32_t*>(p->dev[p->kSeg]);
  hipError_t e = launch_cast_stats_finish(seg, seg + p->nsegs + 1, part, stats, p->nsegs,
                                          to_stream(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "cast plan statistics kernel launch");
}

int byteps_reduce_cast_plan_decompress_stats(byteps_reduce_cast_plan* p, int divisor,
                                             double* stats, void* stream) {
  return cast_plan_stats(p, divisor, stats, stream, false);
}

int byteps_reduce_cast_plan_measure(byteps_reduce_cast_plan* p, int divisor, double* stats,
                                    void* stream) {
  return cast_plan_stats(p, divisor, stats, stream, true);
}

int byteps_reduce_clip_record(const double* rows, int nrows, double max_norm, double eps,
                              const float* inv_scale, byteps_clip_record* out, void* stream) {
  if (nrows < 0) return fail(BYTEPS_REDUCE_EARGS, "nrows %d < 0", nrows);
  if (!rows && nrows > 0) return fail(BYTEPS_REDUCE_EARGS, "null rows pointer");
  if (!out) return fail(BYTEPS_REDUCE_EARGS, "null clip record pointer");
  if ((uintptr_t)out % 8) return fail(BYTEPS_REDUCE_EARGS, "clip record is not 8-byte aligned");
  if (!(max_norm > 0.0) || !std::isfinite(max_norm))
    return fail(BYTEPS_REDUCE_EARGS, "max_norm %g is not a finite positive number", max_norm);
  if (!(eps >= 0.0)) return fail(BYTEPS_REDUCE_EARGS, "eps %g < 0", eps);
  const hipError_t e =
      launch_clip_record(rows, nrows, max_norm, eps, inv_scale, out, to_stream(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "clip record kernel launch");
}

int byteps_reduce_cast_plan_decompress_scaled(byteps_reduce_cast_plan* p, int divisor,
                                              const float* mult, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (const int rc = refuse_sgd(p, "decompress_scaled")) return rc;
  if (divisor < 1) return fail(BYTEPS_REDUCE_EARGS, "divisor %d < 1", divisor);
  if (!mult) return fail(BYTEPS_REDUCE_EARGS, "null mult pointer");
  const uintptr_t mb = (uintptr_t)mult;
  if (mb % sizeof(float)) return fail(BYTEPS_REDUCE_EARGS, "mult is not 4-byte aligned");
  for (const auto& r : p->ranges)
    if (mb < r.second && r.first < mb + sizeof(float))
      return fail(BYTEPS_REDUCE_EARGS, "mult lies inside a segment of the plan");
  if (p->ti.records == 0) return BYTEPS_REDUCE_OK;
  return cast_plan_launch(p, false, divisor, 0, nullptr, stream, false, mult);
}

int byteps_reduce_cast_plan_create_sgd(const byteps_cast_sgd_desc* segs, int nsegs, int wire_dtype,
                                       byteps_reduce_cast_plan** out) {
  return cast_plan_create<unsigned char*>(kCastSgd, segs, nsegs, kFloat32, wire_dtype, out);
}

int byteps_reduce_cast_plan_apply_sgd(byteps_reduce_cast_plan* p, int divisor,
                                      const byteps_sgd_hyper* h, const byteps_clip_record* rec,
                                      int skip_nonfinite, void* stream) {
  if (!p) return fail(BYTEPS_REDUCE_EARGS, "null plan");
  if (p->scheme != kCastSgd)
    return fail(BYTEPS_REDUCE_EARGS,
                "the plan is not an SGD plan (byteps_reduce_cast_plan_create_sgd)");
  if (!h) return fail(BYTEPS_REDUCE_EARGS, "null hyper-parameters");
  if (divisor < 1) return fail(BYTEPS_REDUCE_EARGS, "divisor %d < 1", divisor);
  if (!std::isfinite(h->lr)) return fail(BYTEPS_REDUCE_EARGS, "lr %g is not finite", h->lr);
  if (!(h->momentum >= 0.0f && h->momentum < 1.0f))
    return fail(BYTEPS_REDUCE_EARGS, "momentum %g is not in [0, 1)", h->momentum);
  if (!(h->weight_decay >= 0.0f) || !std::isfinite(h->weight_decay))
    return fail(BYTEPS_REDUCE_EARGS, "weight_decay %g is not a finite number >= 0",
                h->weight_decay);
  if (h->nesterov && h->momentum == 0.0f)
    return fail(BYTEPS_REDUCE_EARGS, "nesterov needs a momentum above 0");
  if (skip_nonfinite && !rec)
    return fail(BYTEPS_REDUCE_EARGS, "skip_nonfinite needs a clip record");
  if (rec) {
    const uintptr_t rb = (uintptr_t)rec;
    if (rb % 8) return fail(BYTEPS_REDUCE_EARGS, "clip record is not 8-byte aligned");
    for (const auto& r : p->ranges)
      if (rb < r.second && r.first < rb + sizeof(byteps_clip_record))
        return fail(BYTEPS_REDUCE_EARGS, "clip record lies inside a segment of the plan");
  }
  if (p->ti.records == 0) return BYTEPS_REDUCE_OK;
  const hipError_t e = p->wire->plan_sgd(
      static_cast<const CastRec*>(p->dev[p->kTable]),
      static_cast<unsigned char* const*>(p->dev[p->kSide]), p->ti.records, divisor, *h, rec,
      skip_nonfinite ? 1 : 0, p->ti.u, p->ti.nelem * 8, tuning(), to_stream(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "SGD plan kernel launch");
}

int byteps_reduce_cast_plan_destroy(byteps_reduce_cast_plan* p) {
  if (!p) return BYTEPS_REDUCE_OK;
  const hipError_t e = cast_plan_free(p);
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "cast plan free");
}

int byteps_reduce_sync(void* stream) {
  hipError_t e = hipStreamSynchronize(to_stream(stream));
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "hipStreamSynchronize");
}

}  // extern "C"
