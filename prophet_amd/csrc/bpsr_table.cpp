// Host arithmetic of the fold launches: element sizes, one fold's geometry and
// the table every batched, planned, block-queue and keyed launch reads.  No
// HIP runtime call (tests/test_table_layout.py builds this file with g++).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "bpsr_api_internal.h"

namespace bpsr {

int elem_size(int dtype) {
  switch (dtype) {
    case kInt8: case kUInt8: return 1;
    case kFloat16: case kBFloat16: return 2;
    case kInt32: case kFloat32: return 4;
    case kInt64: case kFloat64: return 8;
    default: return 0;
  }
}

void make_geom(int dtype, size_t len, const void* dst, const void* const* srcs, int n,
               bool copy_trailing, FoldGeom* g, int* aligned) {
  const uint64_t es = (uint64_t)elem_size(dtype);
  std::memset(g, 0, sizeof(*g));
  g->n_elems = len / es;
  g->trailing_bytes = len % es;
  g->copy_trailing = (copy_trailing && g->trailing_bytes) ? 1u : 0u;
  const uintptr_t d = (uintptr_t)dst;
  bool elem_al = (d % es) == 0, co = true;
  for (int k = 0; k < n; ++k) {
    const uintptr_t s = (uintptr_t)srcs[k];
    elem_al = elem_al && (s % es) == 0;
    co = co && ((s & 15u) == (d & 15u));
  }
  *aligned = elem_al ? 1 : 0;
  // fp16: elements >= floor(n/8)*8 are the reference's scalar tail
  // (cpu_reducer.cc:103 vs :118) and must not enter the vector path.
  const uint64_t vec_end = dtype == kFloat16 ? (g->n_elems / 8) * 8 : g->n_elems;
  g->tail_sem_from = dtype == kFloat16 ? vec_end : g->n_elems;
  if (elem_al && co) {
    uint64_t head = ((16u - (d & 15u)) & 15u) / es;
    if (head > g->n_elems) head = g->n_elems;
    g->head_elems = head;
    g->vec_off = head * es;
    g->nvec = vec_end > head ? ((vec_end - head) * es) / 16 : 0;
    g->tail_begin = head + g->nvec * 16 / es;
  } else {
    g->head_elems = 0;
    g->vec_off = 0;
    g->nvec = 0;
    g->tail_begin = 0;
  }
}

// Element work of one bucket (head, tail, trailing bytes) in parts of
// kElemPart elements per workgroup.
constexpr uint64_t kElemPart = (uint64_t)kBlock * 16;

int build_table(const byteps_bucket_desc* buckets, int nbuckets, int dtype, std::vector<char>& out,
                TableInfo* ti, const int* block_end, int nblocks,
                std::vector<uint32_t>* block_first, int force_vpt) {
  std::vector<BatchEntry> tab;
  std::vector<int> tab_block;  // block of each live bucket
  tab.reserve(nbuckets);
  int blk = 0;
  uint64_t vecs = 0;
  int nmax = 1;
  for (int i = 0; i < nbuckets; ++i) {
    const byteps_bucket_desc& b = buckets[i];
    if (b.n < 1 || b.n > kMaxSrcs)
      return fail(BYTEPS_REDUCE_EARGS, "bucket %d: n=%d outside [1, %d]", i, b.n, kMaxSrcs);
    while (block_end && blk < nblocks && i >= block_end[blk]) ++blk;
    if (b.len == 0) continue;
    if (!b.dst) return fail(BYTEPS_REDUCE_EARGS, "bucket %d: null dst", i);
    for (int k = 0; k < b.n; ++k) {
      if (!b.srcs[k]) return fail(BYTEPS_REDUCE_EARGS, "bucket %d: null srcs[%d]", i, k);
      if (overlaps_partially(b.dst, b.srcs[k], b.len) || (k > 0 && b.srcs[k] == b.dst))
        return fail(BYTEPS_REDUCE_EARGS, "bucket %d: dst overlaps srcs[%d]", i, k);
    }
    BatchEntry e;
    std::memset(&e, 0, sizeof(e));
    for (int k = 0; k < b.n; ++k) e.srcs[k] = static_cast<const unsigned char*>(b.srcs[k]);
    e.dst = static_cast<unsigned char*>(b.dst);
    e.n = b.n;
    make_geom(dtype, b.len, b.dst, b.srcs, b.n, b.dst != b.srcs[0], &e.g, &e.aligned);
    vecs += e.g.nvec;
    nmax = std::max(nmax, b.n);
    tab.push_back(e);
    tab_block.push_back(blk);
  }
  // Same tile-size rule as a single fold (fold_vpt): the tuned vpt, halved
  // while the launch would have fewer than kMinTiles tiles.
  const int vpt = force_vpt ? force_vpt : fold_vpt(vecs, launch_tuning_for_n(nmax).vpt);
  const uint64_t tile_vecs = (uint64_t)kBlock * vpt;
  auto elem_parts = [](const BatchEntry& e) -> uint64_t {
    const uint64_t n_scalar = e.g.head_elems + (e.g.n_elems - e.g.tail_begin);
    const bool trailing = e.g.copy_trailing && e.g.trailing_bytes > 0;
    if (n_scalar == 0 && !trailing) return 0;
    const uint64_t p = (n_scalar + kElemPart - 1) / kElemPart;
    return std::min<uint64_t>(std::max<uint64_t>(p, 1), 65536);
  };
  uint64_t tiles = 0;
  for (auto& e : tab) tiles += elem_parts(e) + (e.g.nvec + tile_vecs - 1) / tile_vecs;
  // grid.x * 256 threads must stay below 2^32
  if (tiles >= (1ull << 32) / kBlock) return fail(BYTEPS_REDUCE_EARGS, "batch too large");
  const uint32_t stride = tile_rec_stride(nmax);
  const size_t recs_off = ((sizeof(BatchEntry) * tab.size()) + 255) & ~(size_t)255;
  out.assign(recs_off + (size_t)stride * tiles, 0);
  if (!tab.empty()) std::memcpy(out.data(), tab.data(), sizeof(BatchEntry) * tab.size());
  char* rec = out.data() + recs_off;
  uint32_t cur_block = 0;
  auto put = [&](unsigned char* dst, uint32_t kind, const BatchEntry& e, uint32_t a, uint32_t b,
                 uint32_t c, uint64_t byte0) {
    TileHead h;
    std::memset(&h, 0, sizeof(h));
    h.dst = dst + byte0;
    h.kind = kind;
    h.n = (uint32_t)e.n;
    h.a = a;
    h.b = b;
    h.c = c;
    h.block = cur_block;
    std::memcpy(rec, &h, sizeof(h));
    const unsigned char** p = reinterpret_cast<const unsigned char**>(rec + kTileHeadBytes);
    for (int k = 0; k < e.n; ++k) p[k] = e.srcs[k] + byte0;
    rec += stride;
  };
  // Records of the live buckets [b0, b1): element tiles first (they are
  // latency-bound and start with the launch), then the vector tiles.
  auto emit = [&](size_t b0, size_t b1) {
    for (size_t b = b0; b < b1; ++b) {
      const uint64_t parts = elem_parts(tab[b]);
      for (uint64_t q = 0; q < parts; ++q)
        put(tab[b].dst, kTileElem, tab[b], (uint32_t)q, (uint32_t)b, (uint32_t)parts, 0);
    }
    for (size_t b = b0; b < b1; ++b) {
      const BatchEntry& e = tab[b];
      for (uint64_t v0 = 0; v0 < e.g.nvec; v0 += tile_vecs) {
        const uint64_t left = e.g.nvec - v0;
        const bool full = left >= tile_vecs;
        put(e.dst, full ? kTileFull : kTilePartial, e, full ? 0u : (uint32_t)left, (uint32_t)b,
            0, e.g.vec_off + v0 * 16);
      }
    }
  };
  char* const rec0 = rec;
  if (!block_end) {
    emit(0, tab.size());
  } else {
    block_first->assign((size_t)nblocks + 1, 0);
    size_t b0 = 0;
    for (int k = 0; k < nblocks; ++k) {
      size_t b1 = b0;
      while (b1 < tab.size() && tab_block[b1] == k) ++b1;
      (*block_first)[k] = (uint32_t)((rec - rec0) / stride);
      cur_block = (uint32_t)k;
      emit(b0, b1);
      b0 = b1;
    }
    (*block_first)[nblocks] = (uint32_t)tiles;
  }
  ti->vpt = vpt;
  ti->nmax = nmax;
  ti->live = (int)tab.size();
  ti->tiles = (uint32_t)tiles;
  ti->rec_stride = stride;
  ti->recs_off = recs_off;
  ti->bytes = out.size();
  return BYTEPS_REDUCE_OK;
}

BatchLaunch batch_launch(const void* dev_table, const TableInfo& ti, bool in_hbm) {
  BatchLaunch L;
  L.entries = static_cast<const BatchEntry*>(dev_table);
  L.recs = static_cast<const unsigned char*>(dev_table) + ti.recs_off;
  L.rec_stride = ti.rec_stride;
  L.tiles = ti.tiles;
  // record prefetch distance (bpsr_kernels_impl.h prefetch_record): one
  // resident round of the 256-CU chip; BPSR_REC_PREFETCH=0 turns it off (A/B)
  static const uint32_t ahead = [] {
    const char* v = getenv("BPSR_REC_PREFETCH");
    const long x = v ? atol(v) : (long)kPrefetchAhead;
    return x > 0 ? (uint32_t)((x + 7) & ~7L) : 0u;  // a multiple of 8: the same XCD
  }();
  L.pf_ahead = in_hbm ? ahead : 0u;
  L.stop = nullptr;
  return L;
}

}  // namespace bpsr
