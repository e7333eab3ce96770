// Host arithmetic of the casts: the operand checks of a single cast
// (cast_check), and of the cast plan (byteps_reduce_cast_plan_*) the table of
// tile records one plan launch reads, compress or decompress, and for an
// error-feedback plan the parallel array of one residual pointer per record,
// for a stochastic-rounding plan that of one (first element index, key) per
// record; and, for the decompress statistics, every segment's records.  No HIP
// runtime call (tests/test_cast_check.py, test_cast_table.py,
// test_cast_table_ef.py, test_cast_table_sr.py and test_cast_table_stats.py
// build this file with g++).
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
// lout: null, or it receives every segment's records and the byte ranges
// tested here (CastSegList).
static int build(const std::vector<Desc>& segs, int wide_dtype, int copy_vpt,
                 std::vector<char>& out, std::vector<unsigned char*>* rout,
                 std::vector<CastSrRec>* sout, CastTableInfo* ti, CastSegList* lout) {
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
    for (const Range& r : ranges) l.ranges.emplace_back(r.begin, r.end);
    *lout = std::move(l);
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

// The three descriptor kinds as Desc.
static Desc desc_of(const byteps_cast_desc& d) { return {d.wide, d.half, nullptr, d.nelem, 0}; }
static Desc desc_of(const byteps_cast_ef_desc& d) { return {d.wide, d.half, d.resid, d.nelem, 0}; }
static Desc desc_of(const byteps_cast_sr_desc& d) {
  return {d.wide, d.half, nullptr, d.nelem, d.key};
}

// What the three builders share ahead of build(): the scheme's dtype rule (a
// table is cut by element size alone, so the fp16 wire stands for both), the
// table's count and pointer, and the descriptors as Desc.
template <class D>
static int build_from(const D* segs, int nsegs, int wide_dtype, CastScheme scheme, int copy_vpt,
                      std::vector<char>& out, std::vector<unsigned char*>* rout,
                      std::vector<CastSrRec>* sout, CastTableInfo* ti, CastSegList* lists) {
  const int rc = cast_dtype_check(kFloat16, wide_dtype, scheme);
  if (rc != BYTEPS_REDUCE_OK) return rc;
  if (nsegs < 0 || (nsegs > 0 && !segs)) return fail(BYTEPS_REDUCE_EARGS, "bad segment table");
  std::vector<Desc> d((size_t)nsegs);
  for (int i = 0; i < nsegs; ++i) d[i] = desc_of(segs[i]);
  return build(d, wide_dtype, copy_vpt, out, rout, sout, ti, lists);
}

int build_cast_table(const byteps_cast_desc* segs, int nsegs, int wide_dtype, int copy_vpt,
                     std::vector<char>& out, CastTableInfo* ti, CastSegList* lists) {
  return build_from(segs, nsegs, wide_dtype, kCastPlain, copy_vpt, out, nullptr, nullptr, ti,
                    lists);
}

int build_cast_table_ef(const byteps_cast_ef_desc* segs, int nsegs, int wide_dtype, int copy_vpt,
                        std::vector<char>& out, std::vector<unsigned char*>& resid_out,
                        CastTableInfo* ti, CastSegList* lists) {
  return build_from(segs, nsegs, wide_dtype, kCastEf, copy_vpt, out, &resid_out, nullptr, ti,
                    lists);
}

int build_cast_table_sr(const byteps_cast_sr_desc* segs, int nsegs, int wide_dtype, int copy_vpt,
                        std::vector<char>& out, std::vector<CastSrRec>& sr_out,
                        CastTableInfo* ti, CastSegList* lists) {
  return build_from(segs, nsegs, wide_dtype, kCastSr, copy_vpt, out, nullptr, &sr_out, ti, lists);
}

int cast_dtype_check(int wire, int wide_dtype, CastScheme scheme) {
  if (wire != kFloat16 && wire != kBFloat16)
    return fail(BYTEPS_REDUCE_EDTYPE, "compression to data type %d", wire);
  if (scheme != kCastPlain) {
    if (wide_dtype != kFloat32)
      return fail(BYTEPS_REDUCE_EDTYPE, "%s compression of data type %d (FLOAT32 only)",
                  scheme == kCastEf ? "error-feedback" : "stochastic-rounding", wide_dtype);
    return BYTEPS_REDUCE_OK;
  }
  const int other = wire == kFloat16 ? kBFloat16 : kFloat16;
  if (wide_dtype != kFloat32 && wide_dtype != kFloat64 && wide_dtype != other)
    return fail(BYTEPS_REDUCE_EDTYPE, "%s compression of data type %d",
                wire == kFloat16 ? "fp16" : "bf16", wide_dtype);
  return BYTEPS_REDUCE_OK;
}

int cast_check(int wire, int wide_dtype, CastScheme scheme, int divisor, size_t nelem,
               const CastOperand* ops, int n) {
  const int rc = cast_dtype_check(wire, wide_dtype, scheme);
  if (rc != BYTEPS_REDUCE_OK) return rc;
  if (divisor < 1) return fail(BYTEPS_REDUCE_EARGS, "divisor %d < 1", divisor);
  if (nelem == 0) return 1;
  for (int i = 0; i < n; ++i)
    if (!ops[i].p) return fail(BYTEPS_REDUCE_EARGS, "null pointer");
  if (scheme == kCastSr && nelem > kSrMaxElems)
    return fail(BYTEPS_REDUCE_EARGS, "more than 2^34 elements");
  for (int i = 0; i < n; ++i)
    if (nelem > SIZE_MAX / ops[i].es) return fail(BYTEPS_REDUCE_EARGS, "element count overflows");
  for (int i = 0; i < n; ++i)
    if ((uintptr_t)ops[i].p > UINTPTR_MAX - nelem * ops[i].es)
      return fail(BYTEPS_REDUCE_EARGS, "operand wraps the address space");
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      const uintptr_t a = (uintptr_t)ops[i].p, b = (uintptr_t)ops[j].p;
      if (a < b + nelem * ops[j].es && b < a + nelem * ops[i].es)
        return fail(BYTEPS_REDUCE_EARGS, "%s and %s overlap", ops[i].name, ops[j].name);
    }
  return BYTEPS_REDUCE_OK;
}

}  // namespace bpsr
