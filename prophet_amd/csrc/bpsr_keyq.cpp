// Keyed block queue (bpsr_internal.h keyq_*): the PS server's device
// releases, on top of the block queue (bpsr_blockq.cpp).
#include <cstdio>

#include "bpsr_api_internal.h"

namespace bpsr {

int keyq_create(const byteps_bucket_desc* buckets, int nkeys, int dtype, double timeout_s,
                byteps_reduce_blockq** out) {
  if (!out || nkeys < 1 || !buckets) return fail(BYTEPS_REDUCE_EARGS, "bad keyed queue table");
  *out = nullptr;
  for (int k = 0; k < nkeys; ++k)
    if (buckets[k].n < 1 || buckets[k].n > kKeyedMaxSrcs)
      return fail(BYTEPS_REDUCE_EARGS, "keyed queue: key %d has %d sources (1..%d)", k,
                  buckets[k].n, kKeyedMaxSrcs);
  std::vector<int> block_end((size_t)nkeys);
  bool wide = false;
  for (int k = 0; k < nkeys; ++k) {
    block_end[(size_t)k] = k + 1;
    wide = wide || buckets[k].n > kKeyedNarrowSrcs;
  }
  byteps_reduce_blockq* q = nullptr;
  int rc = byteps_reduce_blockq_create(buckets, nkeys, block_end.data(), nkeys, dtype,
                                       kModeReference, &q);
  if (rc) return rc;
  q->keyed = true;
  q->wide = wide;
  if (timeout_s > 0) q->timeout_s = timeout_s;
  const size_t nw = (size_t)nkeys * (wide ? 2 : 1);  // words per copy (device / host parity)
  const size_t kbytes = sizeof(uint64_t) * nw * kKeyWordStride;  // one word per line
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&q->kwords), kbytes);
  if (e == hipSuccess) e = hipMemset(q->kwords, 0, kbytes);
  if (e == hipSuccess) e = pinned_words(2 * nw, &q->khwords, &q->khwords_dev);
  const size_t cbytes = sizeof(uint32_t) * (size_t)nkeys * kKeyCntStride;  // one per line
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&q->kcnt), cbytes);
  if (e == hipSuccess) e = hipMemset(q->kcnt, 0, cbytes);
  if (e == hipSuccess) e = pinned_words((size_t)nkeys, &q->khdone, &q->khdone_dev);
  // the host's control word: 256 B, like the device's
  if (e == hipSuccess) e = pinned_words(256 / sizeof(BlockqCtl), &q->hctl, &q->hctl_dev);
  if (e == hipSuccess) e = hipDeviceSynchronize();  // words zeroed before any stream uses them
  if (e != hipSuccess) {
    (void)byteps_reduce_blockq_destroy(q);
    return hip_fail(e, "keyed queue setup");
  }
  *out = q;
  return BYTEPS_REDUCE_OK;
}

int keyq_launch(byteps_reduce_blockq* q, hipEvent_t stop, hipStream_t* stream, uint32_t* epoch) {
  std::lock_guard<std::mutex> g(q->mu);
  hipStream_t own = nullptr;
  hipError_t e = library_queue(q->device, q->cus, 2, &own);
  if (e != hipSuccess) return hip_fail(e, "consumer stream");
  const uint32_t ep = q->launch_epoch + 1;
  // Residency: at most 2 consumer workgroups per CU, and room left beside
  // them for the work a missing release may still need — a push copy into a
  // slot (the copy kernel asks for 40 KiB of LDS) or a release kernel: 58 KiB
  // each (two fit in 160 KiB, three do not; 44 KiB stay free).
  constexpr size_t kKeyedLds = 58u * 1024u;
  int pol = kPolPlain;
  BlockqLaunch Q = blockq_launch_args(q, ep, launch_tuning_for_n(q->ti.nmax), &pol);
  Q.L.stop = stop;
  // (Q.ctl is polled on the device, agent scope)
  Q.herr = &q->hctl_dev->err;    // mirrored to the host by the helper
  Q.helper = 1;  // workgroup 0 forwards the host words
  Q.keyed = 1;
  Q.wide = q->wide ? 1 : 0;
  Q.kwords = q->kwords;
  Q.khwords = q->khwords_dev;
  Q.kcnt = q->kcnt;
  Q.khdone = q->khdone_dev;
  Q.grid = q->ti.tiles + 1;
#ifdef BPSR_KEYED_TRACE
  if (!q->ktrace) {
    q->ktrace_per = 4 * (size_t)q->ti.tiles + (size_t)q->nblocks;
    if (hipMalloc(reinterpret_cast<void**>(&q->ktrace), 8 * q->ktrace_per * kKtraceSlots) != hipSuccess)
      return fail(BYTEPS_REDUCE_EHIP, "keyed trace buffer");
    (void)hipMemset(q->ktrace, 0, 8 * q->ktrace_per * kKtraceSlots);
    (void)hipDeviceSynchronize();
  }
  Q.ktrace = q->ktrace + (size_t)(ep % kKtraceSlots) * q->ktrace_per;
#endif
  ConsumerDev* const D = consumer_dev(q->device);  // (in range: it has a queue set)
  std::lock_guard<std::mutex> dg(D->mu);  // in the device's dispatch sequence
  e = seq_prepare(*D, q->device, Q, own, 4 * Q.timeout_ticks);
  if (e == hipSuccess)
    e = launch_blockq(Q, q->ti.vpt, pol, kKeyedLds, true, q->dtype, q->mode, own);
  if (e != hipSuccess) return hip_fail(e, "keyed queue launch");
  seq_commit(*D, Q, own);
  __atomic_store_n(&q->last_pol, pol, __ATOMIC_RELAXED);
  __atomic_store_n(&q->launch_epoch, ep, __ATOMIC_RELEASE);
  if (stream) *stream = own;
  if (epoch) *epoch = ep;
  return BYTEPS_REDUCE_OK;
}

// A key's release epoch is written only by its releaser (the server
// serialises a key's rounds) and the launch epoch only by keyq_launch (under
// q->mu): both are read lock-free, so releases of different keys from many
// receive threads share no lock.
uint32_t keyq_next_epoch(byteps_reduce_blockq* q, int key) {
  return __atomic_load_n(&q->rel_epoch[(size_t)key], __ATOMIC_ACQUIRE) + 1;
}

bool keyq_advance(byteps_reduce_blockq* q, uint32_t epoch) {
  std::lock_guard<std::mutex> g(q->mu);
  if (q->launch_epoch + 1 != epoch) return false;
  __atomic_store_n(&q->launch_epoch, epoch, __ATOMIC_RELEASE);
  return true;
}

uint32_t keyq_launched(byteps_reduce_blockq* q) {
  return __atomic_load_n(&q->launch_epoch, __ATOMIC_ACQUIRE);
}

void keyq_state(byteps_reduce_blockq* q, int key, uint32_t* next_epoch, uint32_t* launched) {
  *next_epoch = keyq_next_epoch(q, key);
  *launched = keyq_launched(q);
}

int keyq_release(byteps_reduce_blockq* q, int key, uint64_t perm, hipStream_t s, bool* first) {
  const uint32_t ep = q->rel_epoch[(size_t)key] + 1;
  {  // a round (folded here, or a skip word for a lane-folded one): the epoch has begun
    uint32_t o = __atomic_load_n(&q->opened, __ATOMIC_ACQUIRE);
    while (o < ep && !__atomic_compare_exchange_n(&q->opened, &o, ep, true, __ATOMIC_ACQ_REL,
                                                  __ATOMIC_ACQUIRE)) {
    }
    if (first) *first = o < ep;
  }
  const uint64_t w = key_word((uint32_t)perm, ep);
  const uint64_t w2 = key_word((uint32_t)(perm >> 32), ep);  // wide: positions 8..15
  const size_t second = (size_t)q->nblocks + (size_t)key;
  if (s) {
    const hipError_t e =
        launch_key_release(q->kwords, (uint32_t)key * kKeyWordStride, w,
                           q->wide ? q->kwords + second * kKeyWordStride : nullptr, w2, s);
    if (e != hipSuccess) return hip_fail(e, "keyed release");
  } else {
    // the second word first: the helper forwards a block once both carry the epoch
    if (q->wide) __atomic_store_n(q->khwords + 2 * second + (ep & 1u), w2, __ATOMIC_RELEASE);
    __atomic_store_n(q->khwords + 2 * (size_t)key + (ep & 1u), w, __ATOMIC_RELEASE);
  }
  __atomic_store_n(&q->rel_epoch[(size_t)key], ep, __ATOMIC_RELEASE);
  return BYTEPS_REDUCE_OK;
}

uint32_t keyq_opened(const byteps_reduce_blockq* q) {
  return __atomic_load_n(&q->opened, __ATOMIC_ACQUIRE);
}

bool keyq_close(byteps_reduce_blockq* q, uint32_t epoch) {
  uint32_t o = __atomic_load_n(&q->opened, __ATOMIC_ACQUIRE);
  while (o < epoch)
    if (__atomic_compare_exchange_n(&q->opened, &o, epoch, true, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE))
      return true;
  return false;
}

bool keyq_key_done(const byteps_reduce_blockq* q, int key, uint32_t epoch) {
  return epoch_reached(__atomic_load_n(q->khdone + key, __ATOMIC_ACQUIRE), epoch);
}

bool keyq_failed(byteps_reduce_blockq* q) {
  return __atomic_load_n(&q->hctl->err, __ATOMIC_ACQUIRE) != 0;
}

void keyq_shape(const byteps_reduce_blockq* q, uint32_t* tiles, int* vpt, int* pol) {
  *tiles = q->ti.tiles;
  *vpt = q->ti.vpt;
  *pol = __atomic_load_n(&q->last_pol, __ATOMIC_RELAXED);
}

std::string keyq_debug(byteps_reduce_blockq* q) {
  std::lock_guard<std::mutex> g(q->mu);
  std::vector<uint64_t> dev((size_t)q->nblocks);
  const hipError_t e = hipMemcpy2D(dev.data(), 8, q->kwords, 8 * kKeyWordStride, 8, dev.size(),
                                  hipMemcpyDeviceToHost);
  char buf[512];
  int dev_at = 0, rel_at = 0, host_at = 0;
  const uint32_t ep = q->launch_epoch;
  int first_missing = -1;
  for (int b = 0; b < q->nblocks; ++b) {
    if ((uint32_t)dev[(size_t)b] == ep) ++dev_at;
    else if (first_missing < 0) first_missing = b;
    if (q->rel_epoch[(size_t)b] >= ep) ++rel_at;
    const uint64_t h = __atomic_load_n(q->khwords + 2 * (size_t)b + (ep & 1u), __ATOMIC_ACQUIRE);
    if ((uint32_t)h == ep) ++host_at;
  }
  snprintf(buf, sizeof(buf),
           "keyq: launch epoch %u, %d blocks: device words at epoch %d, host releases %d, "
           "host words %d, err %u, copy %d, first missing block %d (device word %llx host %llx)",
           ep, q->nblocks, dev_at, rel_at, host_at, q->hctl->err, (int)e, first_missing,
           first_missing >= 0 ? (unsigned long long)dev[(size_t)first_missing] : 0ull,
           first_missing >= 0 ? (unsigned long long)q->khwords[2 * (size_t)first_missing + (ep & 1u)]
                              : 0ull);
  return buf;
}

}  // namespace bpsr
