// Per device: the library's four hardware queues, their placement on the
// compute pipes, and the dispatch sequence of the block-queue launches
// (bpsr_api_internal.h: ConsumerDev).
#include <cstdlib>

#include "bpsr_api_internal.h"

namespace bpsr {

static std::mutex g_consumer_mu;
static ConsumerDev g_cdev[64];

ConsumerDev* consumer_dev(int device) {
  if (device >= 0 && device < 64) return &g_cdev[device];
  fail(BYTEPS_REDUCE_EARGS, "device %d", device);
  return nullptr;
}

// Makes `device` current for a scope (the current device is per thread).
struct DeviceGuard {
  int prev = -1;  // the device to go back to (-1: none)
  explicit DeviceGuard(int device) {
    (void)hipGetDevice(&prev);
    if (prev == device) prev = -1;
    else (void)hipSetDevice(device);
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// Queue placement (DESIGN.md §4.4 "pipes", round 6).  The hardware serves
// its queues through 4 compute pipes, and queue ids map to pipes as id mod 4
// in every measurement (profiles/r06s01, r06s02, r06s05, r06s07).  A queue on
// the same pipe as a running consumer answers ~2x slower (43 us median
// release kernels instead of 5: the r05s34 segment); the two overlapping
// consumer queues need pipes of their own (on one pipe, overlapped config 3
// fell from 0.80 to 0.74-0.75, r06s07); and the runtime's own normal-priority
// queues serve the server's lanes best one per pipe (the host-resident
// server ran 4.2 ms rounds instead of 3.1 when the library's queues had
// pushed two of them onto one pipe, r06s08-s09).  So the library makes its
// four queues together, one per pipe: consumer queues 0 and 1, the keyed
// consumers' queue 2 and the release queue — its releases never share a pipe
// with a block-queue consumer, and queues made later keep the runtime's
// phase.  If another thread made a queue in between (ids not consecutive),
// the set is completed queue by queue; a queue that does not fit is kept
// idle for a later placement (a destroyed one could reshuffle the hardware's
// queue map).
constexpr uint64_t kPipes = 4;

// g_consumer_mu held, device current.  A new all-CU-masked stream (a hardware
// queue of its own) and the HSA id of its queue.
static hipError_t new_cu_queue(ConsumerDev& D, int cus, hipStream_t* out, uint64_t* id) {
  std::vector<uint32_t> mask((size_t)(cus + 31) / 32, 0u);
  for (int c = 0; c < cus; ++c) mask[(size_t)c / 32] |= 1u << (c % 32);
  hipError_t e = hipSuccess;
  if (!D.idw && (e = pinned_words(8, &D.idw, &D.idw_dev)) != hipSuccess) return e;
  e = hipExtStreamCreateWithCUMask(out, (uint32_t)mask.size(), mask.data());
  if (e == hipSuccess) e = read_queue_id(*out, D.idw_dev);
  if (e == hipSuccess) *id = __atomic_load_n(D.idw, __ATOMIC_ACQUIRE);
  return e;
}

// g_consumer_mu held, device current.  A queue whose id satisfies `fits`:
// an idle spare, or a new one (at most kPipes + 1 tries; the last one made
// is taken if none fits, i.e. the id-to-pipe model did not hold).
template <class Fits>
static hipError_t placed_queue(ConsumerDev& D, int cus, Fits fits, hipStream_t* out, uint64_t* id) {
  for (size_t i = 0; i < D.spare.size(); ++i)
    if (fits(D.spare[i].second)) {
      *out = D.spare[i].first;
      *id = D.spare[i].second;
      D.spare.erase(D.spare.begin() + (long)i);
      return hipSuccess;
    }
  for (uint64_t t = 0;; ++t) {
    hipStream_t s = nullptr;
    uint64_t qid = 0;
    const hipError_t e = new_cu_queue(D, cus, &s, &qid);
    if (e != hipSuccess) return e;
    if (fits(qid) || t == kPipes) {
      *out = s;
      *id = qid;
      return hipSuccess;
    }
    D.spare.push_back({s, qid});
  }
}

// At process exit, before the HIP runtime's own teardown (the handler is
// registered after the runtime is up, and exit handlers run in reverse):
// the library's queues are destroyed like any other stream, not left to the
// runtime's teardown — under rocprofv3 a process holding them at exit faulted
// inside the profiler's own finalizer (profiles/r06s06_exit_fault_frames.txt).
static void destroy_queue_sets() {
  std::lock_guard<std::mutex> g(g_consumer_mu);
  for (auto& D : g_cdev) {
    for (auto& q : D.q)
      if (q) (void)hipStreamDestroy(q), q = nullptr;
    for (auto& sp : D.spare) (void)hipStreamDestroy(sp.first);
    D.spare.clear();
  }
}

// The device's four library queues, made together on first use (above).
static hipError_t queue_set(int device, int cus, ConsumerDev** out) {
  if (!(*out = consumer_dev(device))) return hipErrorInvalidDevice;
  std::lock_guard<std::mutex> g(g_consumer_mu);
  ConsumerDev& D = **out;
  if (D.q[kReleaseQueue]) return hipSuccess;
  DeviceGuard dg(device);
  hipError_t e = hipSuccess;
  for (int k = 0; k < kLibraryQueues && e == hipSuccess; ++k)
    e = new_cu_queue(D, cus, &D.q[k], &D.qid[k]);
  // any queue whose pipe an earlier one of the set has: re-placed
  for (int k = 1; k < kLibraryQueues && e == hipSuccess; ++k) {
    auto taken = [&](uint64_t id) {
      for (int j = 0; j < k; ++j)
        if (D.qid[j] % kPipes == id % kPipes) return true;
      return false;
    };
    if (!taken(D.qid[k])) continue;
    D.spare.push_back({D.q[k], D.qid[k]});
    e = placed_queue(D, cus, [&](uint64_t id) { return !taken(id); }, &D.q[k], &D.qid[k]);
  }
  if (e != hipSuccess) {
    for (auto& q : D.q) q = nullptr;
    return e;
  }
  static bool registered = false;
  if (!registered) registered = std::atexit(destroy_queue_sets) == 0;
  return hipSuccess;
}

hipError_t library_queue(int device, int cus, int k, hipStream_t* out) {
  ConsumerDev* D = nullptr;
  const hipError_t e = queue_set(device, cus, &D);
  if (e == hipSuccess) *out = D->q[k];
  return e;
}

void library_queue_ids(const ConsumerDev* D, uint64_t ids[kLibraryQueues]) {
  std::lock_guard<std::mutex> g(g_consumer_mu);
  for (int k = 0; k < kLibraryQueues; ++k) ids[k] = D->q[k] ? D->qid[k] : 0;
}

// D.mu held.  The started counters, once per device.
static hipError_t seq_init(ConsumerDev& D, int device) {
  if (D.started) return hipSuccess;
  const size_t bytes = 256;
  void* p = nullptr;
  hipError_t e = hipSuccess;
  {
    DeviceGuard dg(device);
    e = hipMalloc(&p, bytes);
    if (e == hipSuccess) e = hipMemset(p, 0, bytes);
    if (e == hipSuccess) e = hipDeviceSynchronize();
  }
  if (e != hipSuccess) {
    if (p) (void)hipFree(p);
    return e;
  }
  D.started = static_cast<unsigned long long*>(p);
  return hipSuccess;
}

// The join entry of stream `s`: its event completes with the latest launch on
// `s` (the launch's stop event), or is recorded on `s` by the next join when
// that launch carried none (a stop event is an end-of-kernel release: ~5 µs
// when another kernel follows on its stream, ~2.4 µs of an overlapped
// iteration; r05s22-23).
hipError_t seq_tail(ConsumerDev& D, hipStream_t s, ConsumerDev::Tail** out) {
  for (auto& t : D.tails)
    if (t.stream == s) {
      *out = &t;
      return hipSuccess;
    }
  // Callers' streams (launches without a queue of their own) come and go:
  // drop entries whose launch has completed and that need no record, so the
  // list stays bounded by the launches still in flight.
  if (D.tails.size() >= 16) {
    size_t k = 0;
    for (auto& t : D.tails) {
      const bool own = t.stream == D.q[0] || t.stream == D.q[1] || t.stream == D.q[2];
      if (!own && !t.record && hipEventQuery(t.ev) == hipSuccess) {
        (void)hipEventDestroy(t.ev);
        continue;
      }
      D.tails[k++] = t;
    }
    D.tails.resize(k);
  }
  hipEvent_t e = nullptr;
  const hipError_t r = hipEventCreateWithFlags(&e, hipEventDisableTiming);
  if (r != hipSuccess) return r;
  D.tails.push_back({s, e, false});
  *out = &D.tails.back();
  return hipSuccess;
}

// Before enqueueing the kernel of a launch on `ls`: put it in the sequence
// and, when the device's previous launch went to another stream, gate `ls`
// until every workgroup launched so far has started (the gate gives up after
// gate_ticks).
hipError_t seq_prepare(ConsumerDev& D, int device, BlockqLaunch& Q, hipStream_t ls,
                       uint64_t gate_ticks) {
  hipError_t e = seq_init(D, device);
  if (e != hipSuccess) return e;
  if (D.any && D.last != ls) e = launch_seq_gate(D.started, D.target, gate_ticks, ls);
  Q.started = D.started;
  return e;
}

// After the kernel was enqueued.
void seq_commit(ConsumerDev& D, const BlockqLaunch& Q, hipStream_t ls) {
  if (!Q.started) return;
  D.target += seq_counted(Q.grid);
  D.last = ls;
  D.any = true;
}

}  // namespace bpsr
