// The block queue of the fold C ABI (include/bpsr/reduce.h,
// byteps_reduce_blockq_*): one launch folds a whole table, each tile once its
// block has been released for the launch's epoch.  Lock order: q->mu before
// the device's ConsumerDev::mu.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "bpsr_api_internal.h"

namespace bpsr {

// q->mu held.  Every block released for `epoch` (host call order).
static bool epoch_released(const byteps_reduce_blockq* q, uint32_t epoch) {
  for (uint32_t r : q->rel_epoch)
    if (!epoch_reached(r, epoch)) return false;
  return true;
}

// q->mu held.  Issue the deferred join-backs whose epochs are fully released
// (all of them when `all`): the caller's stream waits for that launch.
static hipError_t flush_joins(byteps_reduce_blockq* q, bool all) {
  hipError_t e = hipSuccess;
  size_t k = 0;
  for (auto& p : q->pend_join) {
    if (e == hipSuccess && (all || epoch_released(q, p.epoch))) {
      e = hipStreamWaitEvent(p.s, p.ev, 0);
      q->join_evs.push_back(p.ev);  // the wait holds the event's state at this call
      continue;
    }
    q->pend_join[k++] = p;
  }
  q->pend_join.resize(k);
  return e;
}

// q->mu held.  flush_joins for the calls that do nothing else with a stream.
static int issue_joins(byteps_reduce_blockq* q, bool all) {
  if (q->pend_join.empty()) return BYTEPS_REDUCE_OK;
  const hipError_t e = flush_joins(q, all);
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "block queue join-back");
}

// The argument checks of the two range releases.
static int check_blocks(const byteps_reduce_blockq* q, int first, int count) {
  if (!q) return fail(BYTEPS_REDUCE_EARGS, "null block queue");
  if (first < 0 || count < 0 || first > q->nblocks || count > q->nblocks - first)
    return fail(BYTEPS_REDUCE_EARGS, "blocks [%d, %d+%d) outside [0, %d)", first, first, count,
                q->nblocks);
  return BYTEPS_REDUCE_OK;
}

#ifdef BPSR_KEYED_TRACE
// Probe builds: the keyed consumer's stamps to $BPSR_KEYED_TRACE_OUT — a
// header (launch epoch, slots, words per slot, tiles, keys, clock kHz), the
// tiles' first records (block_first), then the slots.
static void dump_ktrace(byteps_reduce_blockq* q) {
  const char* path = getenv("BPSR_KEYED_TRACE_OUT");
  if (!q->ktrace || !path) return;
  (void)hipDeviceSynchronize();
  std::vector<unsigned long long> buf(q->ktrace_per * kKtraceSlots);
  std::vector<uint32_t> bf((size_t)q->nblocks + 1);
  if (hipMemcpy(buf.data(), q->ktrace, 8 * buf.size(), hipMemcpyDeviceToHost) != hipSuccess) return;
  if (hipMemcpy(bf.data(), q->flags + q->nblocks, 4 * bf.size(), hipMemcpyDeviceToHost) != hipSuccess)
    return;
  FILE* f = fopen(path, "wb");
  if (!f) return;
  const unsigned long long hdr[6] = {q->launch_epoch, kKtraceSlots, q->ktrace_per, q->ti.tiles,
                                     (unsigned long long)q->nblocks, q->clock_khz};
  fwrite(hdr, 8, 6, f);
  fwrite(bf.data(), 4, bf.size(), f);
  fwrite(buf.data(), 8, buf.size(), f);
  fclose(f);
}
#endif

static void blockq_free(byteps_reduce_blockq* q) {
#ifdef BPSR_KEYED_TRACE
  dump_ktrace(q);
  if (q->ktrace) (void)hipFree(q->ktrace);
#endif
  // a launch still waiting for releases ends at its timeout at the latest
  for (auto& p : q->pend_join) {
    (void)hipEventSynchronize(p.ev);
    (void)hipEventDestroy(p.ev);
  }
  for (hipEvent_t ev : q->join_evs) (void)hipEventDestroy(ev);
  if (q->kwords) (void)hipFree(q->kwords);
  if (q->khwords) (void)hipHostFree(q->khwords);
  if (q->hctl) (void)hipHostFree(q->hctl);
  if (q->kcnt) (void)hipFree(q->kcnt);
  if (q->khdone) (void)hipHostFree(q->khdone);
  if (q->fork_ev) (void)hipEventDestroy(q->fork_ev);
  if (q->dev_table) (void)hipFree(q->dev_table);
  if (q->flags) (void)hipFree(q->flags);
  if (q->ctl) (void)hipFree(q->ctl);
  if (q->host_err) (void)hipHostFree(q->host_err);
  if (q->hflags) (void)hipHostFree(q->hflags);
  delete q;
}

BlockqLaunch blockq_launch_args(const byteps_reduce_blockq* q, uint32_t epoch, const Tuning& tu,
                                int* pol) {
  BlockqLaunch Q{};
  Q.L = batch_launch(q->dev_table, q->ti);
  Q.flags = q->flags;
  Q.block_first = q->flags + q->nblocks;
  Q.ctl = q->ctl;
  Q.nblocks = (uint32_t)q->nblocks;
  Q.timeout_ticks = (uint64_t)(q->timeout_s * 1e3 * (double)q->clock_khz);
  Q.epoch = epoch;
  *pol = cache_pol(tu, (uint64_t)q->ti.tiles * q->ti.vpt * kBlock * 16);
  return Q;
}

// byteps_reduce_blockq_stream and _release_stream: library queue `k` of the
// queue's device.
static int queue_stream(byteps_reduce_blockq* q, int k, const char* what, void** stream) {
  if (!q || !stream) return fail(BYTEPS_REDUCE_EARGS, "null argument");
  hipStream_t s = nullptr;
  const hipError_t e = library_queue(q->device, q->cus, k, &s);
  if (e != hipSuccess) return hip_fail(e, what);
  *stream = reinterpret_cast<void*>(s);
  return BYTEPS_REDUCE_OK;
}

}  // namespace bpsr

using namespace bpsr;

extern "C" {

int byteps_reduce_blockq_create(const byteps_bucket_desc* buckets, int nbuckets,
                                const int* block_end, int nblocks, int dtype, int mode,
                                byteps_reduce_blockq** out) {
  if (!out) return fail(BYTEPS_REDUCE_EARGS, "null block-queue out-pointer");
  *out = nullptr;
  int rc = check_common(dtype, mode);
  if (rc) return rc;
  if (nbuckets < 0 || (nbuckets > 0 && !buckets))
    return fail(BYTEPS_REDUCE_EARGS, "bad bucket table");
  if (nblocks < 1 || !block_end) return fail(BYTEPS_REDUCE_EARGS, "need >= 1 block");
  for (int k = 0; k < nblocks; ++k) {
    const int lo = k ? block_end[k - 1] : 0;
    if (block_end[k] < lo || block_end[k] > nbuckets)
      return fail(BYTEPS_REDUCE_EARGS, "block_end[%d]=%d not in [%d, %d]", k, block_end[k], lo,
                  nbuckets);
  }
  if (block_end[nblocks - 1] != nbuckets)
    return fail(BYTEPS_REDUCE_EARGS, "last block ends at %d, not at nbuckets=%d",
                block_end[nblocks - 1], nbuckets);
  std::vector<char> host;
  std::vector<uint32_t> first;
  TableInfo ti;
  int gate_occ = 2;
  if (const char* v = getenv("BPSR_BQ_GATE_OCC")) gate_occ = atoi(v);
  if (gate_occ < 1 || gate_occ > 8) gate_occ = 2;
  int force_vpt = 0;  // tile size override for measurements (default: the fold rule)
  if (const char* v = getenv("BPSR_BQ_VPT")) force_vpt = atoi(v);
  if (force_vpt != 1 && force_vpt != 2 && force_vpt != 4) force_vpt = 0;
  if ((rc = build_table(buckets, nbuckets, dtype, host, &ti, block_end, nblocks, &first,
                        force_vpt)))
    return rc;
  auto* q = new byteps_reduce_blockq();
  q->dtype = dtype;
  q->mode = mode;
  q->nblocks = nblocks;
  q->gate_occ = gate_occ;
  q->ti = ti;
  q->rel_epoch.assign((size_t)nblocks, 0u);
  q->host_table = host;
  if (const char* v = getenv("BPSR_BQ_OWN_QUEUE")) q->own_queue = atoi(v) != 0;
  int khz = 0;
  hipError_t e = hipGetDevice(&q->device);
  if (e == hipSuccess)
    e = hipDeviceGetAttribute(&q->cus, hipDeviceAttributeMultiprocessorCount, q->device);
  if (e == hipSuccess)
    e = hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, q->device);
  q->clock_khz = khz > 0 ? (uint64_t)khz : 100000;
  // The release words and the control word get allocations of their own,
  // padded to whole 256-B lines: nothing else may share their cache lines.
  const size_t flag_bytes =
      (sizeof(uint32_t) * (2 * (size_t)nblocks + 1) + 255) & ~(size_t)255;
  if (e == hipSuccess && ti.tiles > 0) e = hipMalloc(&q->dev_table, ti.bytes);
  if (e == hipSuccess && ti.tiles > 0)
    e = hipMemcpy(q->dev_table, host.data(), ti.bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&q->flags), flag_bytes);
  if (e == hipSuccess) e = hipMemset(q->flags, 0, sizeof(uint32_t) * nblocks);
  if (e == hipSuccess)
    e = hipMemcpy(q->flags + nblocks, first.data(), sizeof(uint32_t) * (nblocks + 1),
                  hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&q->ctl), 256);
  if (e == hipSuccess) e = hipMemset(q->ctl, 0, 256);
  if (e == hipSuccess) e = hipDeviceSynchronize();  // words zeroed before any stream uses them
  if (e == hipSuccess)
    e = hipHostMalloc(reinterpret_cast<void**>(&q->host_err), sizeof(uint32_t));
  if (e != hipSuccess) {
    blockq_free(q);
    return hip_fail(e, "block queue setup");
  }
  *out = q;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_blockq_config(byteps_reduce_blockq* q, int wg_per_cu, double timeout_s) {
  if (!q) return fail(BYTEPS_REDUCE_EARGS, "null block queue");
  if (q->keyed && wg_per_cu > 0)
    return fail(BYTEPS_REDUCE_EARGS, "a keyed queue has the dispatch-ordered consumer");
  if (wg_per_cu > 8) return fail(BYTEPS_REDUCE_EARGS, "wg_per_cu %d > 8", wg_per_cu);
  if (wg_per_cu > 0 && q->host_rel)
    return fail(BYTEPS_REDUCE_EARGS, "host releases need the dispatch-ordered consumer");
  if (wg_per_cu > 0 && q->overlap)
    return fail(BYTEPS_REDUCE_EARGS, "overlap needs the dispatch-ordered consumer");
  if (wg_per_cu >= 0) q->occ = wg_per_cu;
  if (timeout_s > 0) q->timeout_s = timeout_s;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_blockq_launch(byteps_reduce_blockq* q, void* stream) {
  if (!q) return fail(BYTEPS_REDUCE_EARGS, "null block queue");
  hipStream_t s = stream_of(stream);
  std::lock_guard<std::mutex> g(q->mu);
  const uint32_t epoch = q->launch_epoch + 1;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusActive) {
    // Host releases write only the pinned words; the helper workgroup that
    // forwards them is left out of a captured launch, so such a launch would
    // wait for its timeout on every replay.
    if (q->host_rel)
      return fail(BYTEPS_REDUCE_EARGS, "captured block-queue launch with host releases on "
                                       "(byteps_reduce_blockq_host_releases(q, 0) first)");
    // A captured launch keeps this epoch in every replay: only iterations
    // whose releases are captured before it (same graph, stream order) replay
    // correctly, so that is what a capture must hold.
    for (int b = 0; b < q->nblocks; ++b)
      if (!epoch_reached(q->rel_epoch[b], epoch))
        return fail(BYTEPS_REDUCE_EARGS,
                    "captured block-queue launch: release every block before the launch "
                    "(block %d is not; epochs are fixed at capture)", b);
  }
  q->launch_epoch = epoch;
  if (q->ti.tiles == 0) return BYTEPS_REDUCE_OK;
  const Tuning tu = launch_tuning_for_n(q->ti.nmax);
  int pol = kPolPlain;
  BlockqLaunch Q = blockq_launch_args(q, epoch, tu, &pol);
  const bool gated = q->occ == 0;
  size_t lds;
  if (gated) {
    // One workgroup per tile.  Residency is capped (LDS) so that workgroups
    // spinning on a release never take a CU's last registers: the release
    // kernels and the copies that precede them must still get onto the CU
    // (at hardware occupancy — 3 of these workgroups per CU — a live release
    // behind H2D copies on another stream never arrived).
    Q.grid = q->ti.tiles;
    if (q->host_rel && cap != hipStreamCaptureStatusActive) {
      Q.helper = 1;  // workgroup 0 forwards host releases (forward_host_releases)
      Q.hflags = q->hflags_dev;
      Q.grid += 1;
    }
    int occ = launch_occ(tu, q->ti.tiles, true);
    if (occ == 0 || occ > q->gate_occ) occ = q->gate_occ;
    lds = occ_lds_bytes(occ);
  } else {
    const uint64_t cap = (uint64_t)q->cus * (uint64_t)q->occ;
    Q.grid = (uint32_t)std::min<uint64_t>(q->ti.tiles, cap);
    // residency cap through LDS (the kernel's own static LDS included)
    lds = ((kLdsPerCU / (size_t)q->occ) - 256) & ~(size_t)255;
  }
  if (cap == hipStreamCaptureStatusActive) {
    // pre-released by rule: runs on the capturing stream, outside the sequence
    const hipError_t e = launch_blockq(Q, q->ti.vpt, pol, lds, gated, q->dtype, q->mode, s);
    return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "block queue kernel launch");
  }
  // The consumer runs on a consumer queue of the device (a hardware queue of
  // its own), forked from `s`; without overlap it runs on queue 0 and joins
  // back into `s`, with overlap it takes the queue the device's previous
  // launch did not and does not join (byteps_reduce_blockq_join).
  ConsumerDev* const D = consumer_dev(q->device);
  if (!D) return BYTEPS_REDUCE_EARGS;
  hipStream_t c0 = nullptr, c1 = nullptr;
  hipError_t e = hipSuccess;
  if (q->own_queue) e = library_queue(q->device, q->cus, 0, &c0);
  if (e == hipSuccess && q->own_queue && q->overlap) e = library_queue(q->device, q->cus, 1, &c1);
  if (e != hipSuccess) return hip_fail(e, "consumer stream");
  std::lock_guard<std::mutex> dg(D->mu);
  hipStream_t ls = s;
  if (q->own_queue) ls = q->overlap && D->last == c0 ? c1 : c0;
  const bool fork = q->own_queue && s != ls && (!q->overlap || (s != c0 && s != c1));
  if (fork) {
    if (!q->fork_ev) e = hipEventCreateWithFlags(&q->fork_ev, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventRecord(q->fork_ev, s);
    if (e == hipSuccess) e = hipStreamWaitEvent(ls, q->fork_ev, 0);
  }
  // The consumer's own completion completes the join event when `s` joins
  // back at once, or when the launch stream is the caller's (a join must not
  // record on a stream the caller may have destroyed since); otherwise the
  // next byteps_reduce_blockq_join records it on the consumer queue (a stop
  // event on every overlapped launch cost 2.4 µs per config-3 iteration:
  // 0.0744 vs 0.0720 ms, r05s23).
  // A launch forked from `s` without overlap joins back into `s` once its
  // epoch is fully released (flush_joins), through a stop event of its own.
  ConsumerDev::Tail* tail = nullptr;
  if (e == hipSuccess) e = seq_tail(*D, ls, &tail);
  const bool join_back = q->own_queue && !q->overlap && s != ls;
  hipEvent_t jev = nullptr;
  if (e == hipSuccess && join_back) {
    if (!q->join_evs.empty()) {
      jev = q->join_evs.back();
      q->join_evs.pop_back();
    } else {
      e = hipEventCreateWithFlags(&jev, hipEventDisableTiming);
    }
  }
  if (e == hipSuccess) {
    const bool stop = !q->own_queue;
    Q.L.stop = join_back ? jev : stop ? tail->ev : nullptr;
    tail->record = !stop;
  }
  if (e == hipSuccess) e = seq_prepare(*D, q->device, Q, ls, 4 * Q.timeout_ticks);
  if (e == hipSuccess) e = launch_blockq(Q, q->ti.vpt, pol, lds, gated, q->dtype, q->mode, ls);
  if (e == hipSuccess) seq_commit(*D, Q, ls);
  if (e == hipSuccess && join_back) {
    q->pend_join.push_back({s, jev, epoch});
    e = flush_joins(q, false);  // a pre-released epoch joins at once
  } else if (jev) {
    q->join_evs.push_back(jev);
  }
  return e == hipSuccess ? BYTEPS_REDUCE_OK : hip_fail(e, "block queue kernel launch");
}

int byteps_reduce_blockq_overlap(byteps_reduce_blockq* q, int on) {
  if (!q) return fail(BYTEPS_REDUCE_EARGS, "null block queue");
  std::lock_guard<std::mutex> g(q->mu);
  if (!on) {
    q->overlap = false;
    return BYTEPS_REDUCE_OK;
  }
  if (q->keyed || q->occ != 0)
    return fail(BYTEPS_REDUCE_EARGS, "overlap needs the dispatch-ordered consumer "
                                     "(byteps_reduce_blockq_config wg_per_cu = 0)");
  if (!consumer_dev(q->device)) return BYTEPS_REDUCE_EARGS;
  q->overlap = true;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_blockq_join(byteps_reduce_blockq* q, void* stream) {
  if (!q) return fail(BYTEPS_REDUCE_EARGS, "null block queue");
  ConsumerDev* const D = consumer_dev(q->device);
  if (!D) return BYTEPS_REDUCE_EARGS;
  hipStream_t s = stream_of(stream);
  std::lock_guard<std::mutex> g(q->mu);  // (q->mu before D->mu, as in launch)
  if (const int rc = issue_joins(q, true)) return rc;
  std::lock_guard<std::mutex> dg(D->mu);
  for (auto& t : D->tails) {
    if (t.stream == s) continue;
    hipError_t e = hipSuccess;
    if (t.record) e = hipEventRecord(t.ev, t.stream);
    t.record = false;
    if (e == hipSuccess) e = hipStreamWaitEvent(s, t.ev, 0);
    if (e != hipSuccess) return hip_fail(e, "block queue join");
  }
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_blockq_release_range(byteps_reduce_blockq* q, int first, int count,
                                       void* stream) {
  if (const int rc = check_blocks(q, first, count)) return rc;
  hipStream_t s = stream_of(stream);
  std::lock_guard<std::mutex> g(q->mu);
  // Each block's release carries its own next epoch; a range whose blocks are
  // at different epochs (a block released ahead) goes out as one kernel per
  // run of equal epochs.  A one-wave kernel raises the words at system scope:
  // a hipMemset node was not seen by the consumer's polls under graph replay,
  // and hipStreamWriteValue32, copy-engine copies, host functions and events
  // measured no better for per-block releases.
  int b = first;
  const int end = first + count;
  while (b < end) {
    const uint32_t ep = q->rel_epoch[b] + 1;
    int run = b + 1;
    while (run < end && q->rel_epoch[run] + 1 == ep) ++run;
    const hipError_t e = launch_blockq_release(q->flags, (uint32_t)b, (uint32_t)(run - b), ep, s);
    if (e != hipSuccess) return hip_fail(e, "block release");
    for (int k = b; k < run; ++k) q->rel_epoch[k] = ep;
    b = run;
  }
  return issue_joins(q, false);
}

int byteps_reduce_blockq_host_releases(byteps_reduce_blockq* q, int on) {
  if (!q) return fail(BYTEPS_REDUCE_EARGS, "null block queue");
  std::lock_guard<std::mutex> g(q->mu);
  if (!on) {
    q->host_rel = false;
    return BYTEPS_REDUCE_OK;
  }
  if (q->occ != 0)
    return fail(BYTEPS_REDUCE_EARGS, "host releases need the dispatch-ordered consumer "
                                     "(byteps_reduce_blockq_config wg_per_cu = 0)");
  if (!q->hflags) {
    // 0 = never released from the host (the helper skips such words)
    const char* step = "";
    const hipError_t e = pinned_words((size_t)q->nblocks, &q->hflags, &q->hflags_dev, &step);
    if (e != hipSuccess)
      return fail(BYTEPS_REDUCE_EHIP, "%s(host release words): %s", step, hipGetErrorString(e));
  }
  q->host_rel = true;
  return BYTEPS_REDUCE_OK;
}

int byteps_reduce_blockq_release_host(byteps_reduce_blockq* q, int first, int count) {
  if (const int rc = check_blocks(q, first, count)) return rc;
  std::lock_guard<std::mutex> g(q->mu);
  if (!q->host_rel)
    return fail(BYTEPS_REDUCE_EARGS, "host releases not enabled (byteps_reduce_blockq_host_releases)");
  // Each block's word carries its own next epoch (as release_range); the
  // caller's data is complete before the call, so a release store suffices.
  for (int b = first; b < first + count; ++b) {
    const uint32_t ep = q->rel_epoch[b] + 1;
    q->rel_epoch[b] = ep;
    __atomic_store_n(q->hflags + b, ep, __ATOMIC_RELEASE);
  }
  return issue_joins(q, false);
}

int byteps_reduce_blockq_release(byteps_reduce_blockq* q, int block, void* stream) {
  if (!q) return fail(BYTEPS_REDUCE_EARGS, "null block queue");
  if (block >= q->nblocks) return fail(BYTEPS_REDUCE_EARGS, "block %d >= %d", block, q->nblocks);
  return block < 0 ? byteps_reduce_blockq_release_range(q, 0, q->nblocks, stream)
                   : byteps_reduce_blockq_release_range(q, block, 1, stream);
}

int byteps_reduce_blockq_status(byteps_reduce_blockq* q, void* stream) {
  if (!q) return fail(BYTEPS_REDUCE_EARGS, "null block queue");
  hipStream_t s = stream_of(stream);
  if (q->overlap) {  // launches do not join their stream: the status waits for all of them
    if (const int rc = byteps_reduce_blockq_join(q, stream)) return rc;
  } else {           // deferred join-backs go out now (their launch streams wait)
    std::lock_guard<std::mutex> g(q->mu);
    if (const int rc = issue_joins(q, true)) return rc;
  }
  hipError_t e = hipMemcpyAsync(q->host_err, &q->ctl->err, sizeof(uint32_t),
                                hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e, "block queue status");
  if (*q->host_err == 0) return BYTEPS_REDUCE_OK;
  e = hipMemsetAsync(&q->ctl->err, 0, sizeof(uint32_t), s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) return hip_fail(e, "block queue status reset");
  {
    // The abandoned iteration's missing releases will not come: count them as
    // given, so the next iteration's releases carry the next launch's epoch.
    std::lock_guard<std::mutex> g(q->mu);
    for (auto& r : q->rel_epoch)
      if (!epoch_reached(r, q->launch_epoch)) r = q->launch_epoch;
  }
  return fail(BYTEPS_REDUCE_ETIMEOUT,
              "block queue: a block was not released within %.3f s; the launch stopped early",
              q->timeout_s);
}

int byteps_reduce_blockq_stream(byteps_reduce_blockq* q, void** stream) {
  return queue_stream(q, 0, "consumer stream", stream);
}

int byteps_reduce_blockq_release_stream(byteps_reduce_blockq* q, void** stream) {
  return queue_stream(q, kReleaseQueue, "release stream", stream);
}

int byteps_reduce_blockq_queue_ids(byteps_reduce_blockq* q, uint64_t* ids, int cap) {
  if (!q || !ids || cap < 4) return fail(BYTEPS_REDUCE_EARGS, "null argument or cap < 4");
  const ConsumerDev* const D = consumer_dev(q->device);
  if (!D) return BYTEPS_REDUCE_EARGS;
  library_queue_ids(D, ids);
  return kLibraryQueues;
}

int byteps_reduce_blockq_debug(byteps_reduce_blockq* q, uint32_t* out, int cap) {
  if (!q || !out) return fail(BYTEPS_REDUCE_EARGS, "null argument");
  const int nb = q->nblocks;
  const int need = 3 + 3 * nb + 1;
  if (cap < need) return fail(BYTEPS_REDUCE_EARGS, "cap %d < %d", cap, need);
  hipError_t e = hipDeviceSynchronize();
  std::vector<uint32_t> dev(2 * (size_t)nb + 1);
  if (e == hipSuccess) e = hipMemcpy(dev.data(), q->flags, dev.size() * 4, hipMemcpyDeviceToHost);
  uint32_t err = 0;
  if (e == hipSuccess) e = hipMemcpy(&err, &q->ctl->err, 4, hipMemcpyDeviceToHost);
  std::vector<char> tab(q->host_table.size());
  if (e == hipSuccess && !tab.empty())
    e = hipMemcpy(tab.data(), q->dev_table, tab.size(), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return hip_fail(e, "blockq debug");
  std::lock_guard<std::mutex> g(q->mu);
  int k = 0;
  out[k++] = q->launch_epoch;
  out[k++] = (uint32_t)nb;
  out[k++] = err;
  for (int b = 0; b < nb; ++b) out[k++] = q->rel_epoch[b];
  for (size_t i = 0; i < dev.size(); ++i) out[k++] = dev[i];   // words, then block_first
  out[k++] = tab == q->host_table ? 1u : 0u;
  return k;
}

int byteps_reduce_blockq_destroy(byteps_reduce_blockq* q) {
  if (q) blockq_free(q);
  return BYTEPS_REDUCE_OK;
}

}  // extern "C"
