// Host arithmetic of the cast plan (byteps_reduce_cast_plan_*): the table of
// tile records one plan launch reads, compress or decompress.  No HIP runtime
// call (tests/test_cast_table.py builds this file with g++).
#include <algorithm>
#include <cstring>

#include "bpsr_api_internal.h"

namespace bpsr {

namespace {

struct Seg {
  unsigned char* wide;
  unsigned char* half;
  uint64_t nelem;
  CastCut cut;
};

struct Range {
  uintptr_t begin, end;
  int seg;
};

}  // namespace

int build_cast_table(const byteps_cast_desc* segs, int nsegs, int wide_dtype, int copy_vpt,
                     std::vector<char>& out, CastTableInfo* ti) {
  if (wide_dtype != kFloat32 && wide_dtype != kFloat64 && wide_dtype != kBFloat16)
    return fail(BYTEPS_REDUCE_EDTYPE, "fp16 compression of data type %d", wide_dtype);
  if (nsegs < 0 || (nsegs > 0 && !segs)) return fail(BYTEPS_REDUCE_EARGS, "bad segment table");
  const uint64_t es = (uint64_t)elem_size(wide_dtype);
  std::vector<Seg> live;
  std::vector<Range> ranges;
  live.reserve((size_t)nsegs);
  ranges.reserve(2 * (size_t)nsegs);
  uint64_t total = 0;
  for (int i = 0; i < nsegs; ++i) {
    const byteps_cast_desc& d = segs[i];
    if (d.nelem == 0) continue;
    if (!d.wide || !d.half) return fail(BYTEPS_REDUCE_EARGS, "segment %d: null pointer", i);
    if (d.nelem > SIZE_MAX / es)
      return fail(BYTEPS_REDUCE_EARGS, "segment %d: element count overflows", i);
    const uintptr_t w = (uintptr_t)d.wide, h = (uintptr_t)d.half;
    const size_t wb = d.nelem * es, hb = d.nelem * 2;
    if (w > UINTPTR_MAX - wb || h > UINTPTR_MAX - hb)
      return fail(BYTEPS_REDUCE_EARGS, "segment %d: operand wraps the address space", i);
    if (total > UINT64_MAX - d.nelem) return fail(BYTEPS_REDUCE_EARGS, "plan too large");
    total += d.nelem;
    ranges.push_back({w, w + wb, i});
    ranges.push_back({h, h + hb, i});
    live.push_back({static_cast<unsigned char*>(d.wide), static_cast<unsigned char*>(d.half),
                    (uint64_t)d.nelem, cast_cut(d.half, d.wide, d.nelem, (int)es)});
  }
  // The plan serves both directions, so every range is written in one of
  // them: all 2 * live ranges must be pairwise disjoint.  Sorted by their
  // first byte, two ranges overlap iff some range starts before the furthest
  // end seen so far.
  std::sort(ranges.begin(), ranges.end(),
            [](const Range& a, const Range& b) { return a.begin < b.begin; });
  for (size_t k = 1, far = 0; k < ranges.size(); ++k) {
    if (ranges[k].begin < ranges[far].end)
      return fail(BYTEPS_REDUCE_EARGS, "segments %d and %d overlap", ranges[far].seg,
                  ranges[k].seg);
    if (ranges[k].end > ranges[far].end) far = k;
  }
  // The single cast's tile-size rule (launch_cast), over the whole launch.
  auto tiles = [&live](int u) {
    const uint64_t tile = (uint64_t)kBlock * (uint64_t)u;
    uint64_t t = 0;
    for (const Seg& s : live) t += (s.cut.nunits + tile - 1) / tile;
    return t;
  };
  int u = copy_vpt == 1 || copy_vpt == 4 ? copy_vpt : 2;
  while (u > 1 && tiles(u) < kMinTiles) u >>= 1;
  const uint64_t tile_units = (uint64_t)kBlock * (uint64_t)u;
  auto parts = [](uint64_t n) { return (n + kCastElemPart - 1) / kCastElemPart; };
  uint64_t records = tiles(u);
  for (const Seg& s : live) {
    if (s.cut.nunits == 0) {
      records += parts(s.nelem);
    } else {
      const uint64_t tail = s.nelem - (s.cut.head + 8 * s.cut.nunits);
      records += (s.cut.head ? 1 : 0) + (tail ? 1 : 0);
    }
  }
  if (records >= (1ull << 31)) return fail(BYTEPS_REDUCE_EARGS, "plan too large");
  std::vector<char> tab((size_t)records * sizeof(CastRec), 0);
  char* rec = tab.data();
  // `first` elements into the segment, `count` units (vector tiles) or
  // elements (element ranges)
  auto put = [&](const Seg& s, uint32_t kind, uint64_t first, uint64_t count) {
    CastRec r;
    std::memset(&r, 0, sizeof(r));
    r.wide = s.wide + first * es;
    r.half = s.half + first * 2;
    r.kind = kind;
    r.count = (uint32_t)count;
    r.aligned = (uint32_t)s.cut.aligned;
    std::memcpy(rec, &r, sizeof(r));
    rec += sizeof(r);
  };
  for (const Seg& s : live) {
    if (s.cut.nunits == 0) {
      for (uint64_t e = 0; e < s.nelem; e += kCastElemPart)
        put(s, kTileElem, e, std::min<uint64_t>(kCastElemPart, s.nelem - e));
      continue;
    }
    const uint64_t tail_begin = s.cut.head + 8 * s.cut.nunits;
    if (s.cut.head) put(s, kTileElem, 0, s.cut.head);
    if (tail_begin < s.nelem) put(s, kTileElem, tail_begin, s.nelem - tail_begin);
    const uint64_t full = s.cut.nunits / tile_units;
    if (full * tile_units < s.cut.nunits)
      put(s, kTilePartial, s.cut.head + 8 * full * tile_units, s.cut.nunits - full * tile_units);
  }
  for (const Seg& s : live)
    for (uint64_t t = 0; t < s.cut.nunits / tile_units; ++t)
      put(s, kTileFull, s.cut.head + 8 * t * tile_units, tile_units);
  out.swap(tab);
  ti->u = u;
  ti->live = (int)live.size();
  ti->records = (uint32_t)records;
  ti->nelem = total;
  ti->bytes = out.size();
  return BYTEPS_REDUCE_OK;
}

}  // namespace bpsr
