// Host arithmetic of the cast plan (byteps_reduce_cast_plan_*): the table of
// tile records one plan launch reads, compress or decompress, and for an
// error-feedback plan the parallel array of one residual pointer per record,
// for a stochastic-rounding plan that of one (first element index, key) per
// record; and, for the decompress statistics, every segment's records.  No HIP
// runtime call (tests/test_cast_table.py, test_cast_table_ef.py,
// test_cast_table_sr.py and test_cast_table_stats.py build this file with g++).
#include <algorithm>
#include <cstring>

#include "bpsr_api_internal.h"

namespace bpsr {

namespace {

// byteps_cast_desc, byteps_cast_ef_desc and byteps_cast_sr_desc as one: resid
// is null without error feedback, key is 0 without stochastic rounding
struct Desc {
  void* wide;
  void* half;
  void* resid;
  size_t nelem;
  uint32_t key;
};

struct Seg {
  unsigned char* wide;
  unsigned char* half;
  unsigned char* resid;  // error-feedback plans, else null
  uint64_t nelem;
  CastCut cut;
  uint32_t key;          // stochastic-rounding plans, else 0
  int index;             // the segment's place in the caller's table
};

struct Range {
  uintptr_t begin, end;
  int seg;
};

}  // namespace

// rout: null for a plain plan; for an error-feedback plan (f32 wide side) it
// receives one residual pointer per record, the segment's residual base plus
// the record's distance into the wide operand — wide and residual are both
// f32, so the byte offsets agree.
// sout: null but for a stochastic-rounding plan; it receives per record the
// index in its segment of the record's first element and the segment's key,
// and a segment of more than kSrMaxElems elements is an error.
// lout: null, or it receives every segment's records (CastSegList).
static int build(const std::vector<Desc>& segs, int wide_dtype, int copy_vpt,
                 std::vector<char>& out, std::vector<unsigned char*>* rout,
                 std::vector<CastSrRec>* sout, CastTableInfo* ti, CastSegList* lout = nullptr) {
  const int nsegs = (int)segs.size();
  const bool ef = rout != nullptr;
  const uint64_t es = (uint64_t)elem_size(wide_dtype);
  std::vector<Seg> live;
  std::vector<Range> ranges;
  live.reserve((size_t)nsegs);
  ranges.reserve((ef ? 3 : 2) * (size_t)nsegs);
  uint64_t total = 0;
  for (int i = 0; i < nsegs; ++i) {
    const Desc& d = segs[i];
    if (d.nelem == 0) continue;
    if (!d.wide || !d.half || (ef && !d.resid))
      return fail(BYTEPS_REDUCE_EARGS, "segment %d: null pointer", i);
    if (d.nelem > SIZE_MAX / es)
      return fail(BYTEPS_REDUCE_EARGS, "segment %d: element count overflows", i);
    if (sout && d.nelem > kSrMaxElems)
      return fail(BYTEPS_REDUCE_EARGS, "segment %d: more than 2^34 elements", i);
    const uintptr_t w = (uintptr_t)d.wide, h = (uintptr_t)d.half;
    const size_t wb = d.nelem * es, hb = d.nelem * 2;
    if (w > UINTPTR_MAX - wb || h > UINTPTR_MAX - hb || (ef && (uintptr_t)d.resid > UINTPTR_MAX - wb))
      return fail(BYTEPS_REDUCE_EARGS, "segment %d: operand wraps the address space", i);
    if (total > UINT64_MAX - d.nelem) return fail(BYTEPS_REDUCE_EARGS, "plan too large");
    total += d.nelem;
    ranges.push_back({w, w + wb, i});
    ranges.push_back({h, h + hb, i});
    if (ef) ranges.push_back({(uintptr_t)d.resid, (uintptr_t)d.resid + wb, i});
    live.push_back({static_cast<unsigned char*>(d.wide), static_cast<unsigned char*>(d.half),
                    static_cast<unsigned char*>(d.resid), (uint64_t)d.nelem,
                    ef ? cast_cut_ef(d.half, d.wide, d.resid, d.nelem)
                       : cast_cut(d.half, d.wide, d.nelem, (int)es),
                    d.key, i});
  }
  // The plan serves both directions, so every range is written in one of
  // them (the residual by the compress): all 2 * live ranges (3 * live with
  // residuals) must be pairwise disjoint.  Sorted by their
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
  std::vector<unsigned char*> rtab;
  if (ef) rtab.reserve((size_t)records);
  std::vector<CastSrRec> stab;
  if (sout) stab.reserve((size_t)records);
  std::vector<uint32_t> owner;  // the segment of every record, as emitted
  if (lout) owner.reserve((size_t)records);
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
    if (ef) rtab.push_back(s.resid + first * es);
    if (sout) stab.push_back(CastSrRec{first, s.key, 0});
    if (lout) owner.push_back((uint32_t)s.index);
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
  if (lout) {
    // counting sort by segment: stable, so a segment's records stay ascending
    CastSegList l;
    l.seg_begin.assign((size_t)nsegs + 1, 0);
    for (uint32_t o : owner) ++l.seg_begin[(size_t)o + 1];
    for (int i = 0; i < nsegs; ++i) l.seg_begin[(size_t)i + 1] += l.seg_begin[(size_t)i];
    l.seg_recs.resize(owner.size());
    std::vector<uint32_t> at(l.seg_begin.begin(), l.seg_begin.end() - 1);
    for (uint32_t r = 0; r < (uint32_t)owner.size(); ++r) l.seg_recs[at[owner[r]]++] = r;
    lout->seg_begin.swap(l.seg_begin);
    lout->seg_recs.swap(l.seg_recs);
  }
  out.swap(tab);
  if (ef) rout->swap(rtab);
  if (sout) sout->swap(stab);
  ti->u = u;
  ti->live = (int)live.size();
  ti->records = (uint32_t)records;
  ti->nelem = total;
  ti->bytes = out.size();
  return BYTEPS_REDUCE_OK;
}

int build_cast_table(const byteps_cast_desc* segs, int nsegs, int wide_dtype, int copy_vpt,
                     std::vector<char>& out, CastTableInfo* ti) {
  return build_cast_table(segs, nsegs, wide_dtype, copy_vpt, out, ti, nullptr);
}

int build_cast_table(const byteps_cast_desc* segs, int nsegs, int wide_dtype, int copy_vpt,
                     std::vector<char>& out, CastTableInfo* ti, CastSegList* lists) {
  if (wide_dtype != kFloat32 && wide_dtype != kFloat64 && wide_dtype != kBFloat16)
    return fail(BYTEPS_REDUCE_EDTYPE, "fp16 compression of data type %d", wide_dtype);
  if (nsegs < 0 || (nsegs > 0 && !segs)) return fail(BYTEPS_REDUCE_EARGS, "bad segment table");
  std::vector<Desc> d((size_t)nsegs);
  for (int i = 0; i < nsegs; ++i) d[i] = {segs[i].wide, segs[i].half, nullptr, segs[i].nelem, 0};
  return build(d, wide_dtype, copy_vpt, out, nullptr, nullptr, ti, lists);
}

int build_cast_table_ef(const byteps_cast_ef_desc* segs, int nsegs, int wide_dtype, int copy_vpt,
                        std::vector<char>& out, std::vector<unsigned char*>& resid_out,
                        CastTableInfo* ti) {
  return build_cast_table_ef(segs, nsegs, wide_dtype, copy_vpt, out, resid_out, ti, nullptr);
}

int build_cast_table_ef(const byteps_cast_ef_desc* segs, int nsegs, int wide_dtype, int copy_vpt,
                        std::vector<char>& out, std::vector<unsigned char*>& resid_out,
                        CastTableInfo* ti, CastSegList* lists) {
  if (wide_dtype != kFloat32)
    return fail(BYTEPS_REDUCE_EDTYPE, "error-feedback compression of data type %d (FLOAT32 only)",
                wide_dtype);
  if (nsegs < 0 || (nsegs > 0 && !segs)) return fail(BYTEPS_REDUCE_EARGS, "bad segment table");
  std::vector<Desc> d((size_t)nsegs);
  for (int i = 0; i < nsegs; ++i)
    d[i] = {segs[i].wide, segs[i].half, segs[i].resid, segs[i].nelem, 0};
  return build(d, wide_dtype, copy_vpt, out, &resid_out, nullptr, ti, lists);
}

int build_cast_table_sr(const byteps_cast_sr_desc* segs, int nsegs, int wide_dtype, int copy_vpt,
                        std::vector<char>& out, std::vector<CastSrRec>& sr_out,
                        CastTableInfo* ti) {
  return build_cast_table_sr(segs, nsegs, wide_dtype, copy_vpt, out, sr_out, ti, nullptr);
}

int build_cast_table_sr(const byteps_cast_sr_desc* segs, int nsegs, int wide_dtype, int copy_vpt,
                        std::vector<char>& out, std::vector<CastSrRec>& sr_out,
                        CastTableInfo* ti, CastSegList* lists) {
  if (wide_dtype != kFloat32)
    return fail(BYTEPS_REDUCE_EDTYPE,
                "stochastic-rounding compression of data type %d (FLOAT32 only)", wide_dtype);
  if (nsegs < 0 || (nsegs > 0 && !segs)) return fail(BYTEPS_REDUCE_EARGS, "bad segment table");
  std::vector<Desc> d((size_t)nsegs);
  for (int i = 0; i < nsegs; ++i)
    d[i] = {segs[i].wide, segs[i].half, nullptr, segs[i].nelem, segs[i].key};
  return build(d, wide_dtype, copy_vpt, out, nullptr, &sr_out, ti, lists);
}

}  // namespace bpsr
