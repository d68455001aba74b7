// mpjx_indexed_plan.hpp — the irregular derived datatypes (Hvector, Indexed, Hindexed, Struct with the LB / UB
// markers: struct_form, BoundsAcc) and the host-side planning of k_indexed (mpjx_k_indexed.hip). No HIP include:
// plain C++17, compiled, tested and sanitized on the CPU (tests/cpp/indexed_plan_test.cpp); the kernel includes
// the same header, so the address function the test walks is the one the kernel runs.
//
// An irregular type is a list of blocks (offset, length) in base elements from the item's origin, in PACK
// order: the order of the constructor's arrays, as Indexed.IndexedPacker.pack walks them, not address order
// (src/mpi/Indexed.java:61-178, src/mpi/Vector.java:65-135). Its bounds are the reference's:
//   size = sum bl * old.size         lb = min over non-empty blocks of (start + old.lb)
//   extent = ub - lb                 ub = max over non-empty blocks of (start + (bl - 1) * old.extent + old.ub)
// Item k of a message starts k * extent after item 0's origin and block offsets are added to that origin: lb is
// NOT subtracted (GenericPacker), so Indexed([2],[3],INT) has lb 3, extent 2 and its item k is elements
// 3 + 2k, 4 + 2k past the buffer position. A non-contiguous oldtype is flattened into the list here;
// consecutive blocks that abut in pack order AND address order are merged; zero-length blocks are dropped.
// A list that is regular (equal lengths at a constant positive stride of at least the length, first offset 0)
// normalises to the regular TypeForm and takes exactly k_strided's or k_moves' path.
//
// The kernel sees an irregular side as a device table of IdxEnt {byte offset, packed-byte prefix} per block
// and finds the block of a packed byte by a binary search of the prefix (indexed_addr).
#pragma once
#include "mpjx_strided_plan.hpp"

namespace mpjx {

constexpr int64_t kIndexedMaxBlocks = (int64_t)1 << 20;  // merged blocks per type: a 16 MiB device table

// ---- construction -----------------------------------------------------------------------------------------

// Block b of one item of `f` (any form), in base elements
inline int64_t form_nblocks(const TypeForm& f) { return f.irr ? (int64_t)f.irr->tab.size() : f.nblocks; }
inline void form_block(const TypeForm& f, int64_t b, int64_t* off, int64_t* len) {
  if (f.irr) {
    *off = f.irr->tab[(size_t)b].off / f.bsz;
    *len = f.irr->len((size_t)b) / f.bsz;
  } else {
    *off = b * f.stride;
    *len = f.blocklen;
  }
}

struct ElemBlock {
  int64_t off, len;  // base elements
};

// The form of `blocks` (pack order, merged, none empty), regular where the list is, with the reference's bounds
// lb, ub and sticky flags (TypeForm::set_bounds: kept apart only where they are not the blocks' own). The
// irregular layout's own lb and ub are the blocks' — the lowest and one past the highest element touched —
// which is what SideBytes::span() reports.
inline void normal_form(const TypeForm& old, const std::vector<ElemBlock>& v, int64_t rlb, int64_t rub, bool lbs,
                        bool ubs, TypeForm* out) {
  *out = contiguous_form(old.base, old.bsz, 0);
  if (v.empty()) {
    out->set_bounds(rlb, rub, lbs, ubs);
    return;
  }
  int64_t lb = v[0].off, ub = v[0].off + v[0].len;
  for (const ElemBlock& b : v) lb = std::min(lb, b.off), ub = std::max(ub, b.off + b.len);
  bool reg = v[0].off == 0;
  const int64_t st = v.size() > 1 ? v[1].off - v[0].off : v[0].len;
  for (size_t i = 1; reg && i < v.size(); i++) reg = v[i].len == v[0].len && v[i].off - v[i - 1].off == st;
  if (reg && st >= v[0].len) {
    out->nblocks = (int64_t)v.size();
    out->blocklen = v[0].len;
    out->stride = st;
    out->set_bounds(rlb, rub, lbs, ubs);
    return;
  }
  auto irr = std::make_shared<IrrLayout>();
  const int64_t bsz = old.bsz;
  irr->tab.reserve(v.size());
  uint64_t pre = 0, mask = (uint64_t)((ub - lb) * bsz);
  for (const ElemBlock& b : v) {
    irr->tab.push_back(IdxEnt{b.off * bsz, pre});
    pre += (uint64_t)(b.len * bsz);
    mask |= (uint64_t)(b.off * bsz) | (uint64_t)(b.len * bsz);
  }
  irr->size = (int64_t)pre;
  irr->lb = lb * bsz;
  irr->ub = ub * bsz;
  irr->amask = mask;
  std::vector<ElemBlock> s(v);
  std::sort(s.begin(), s.end(), [](const ElemBlock& a, const ElemBlock& b) { return a.off < b.off; });
  for (size_t i = 1; i < s.size() && !irr->self_overlap; i++) irr->self_overlap = s[i - 1].off + s[i - 1].len > s[i].off;
  out->irr = irr;
  out->set_bounds(rlb, rub, lbs, ubs);
}

// The bounds of a type from its blocks, by the reference's rules. Indexed / Hindexed / Vector / Hvector /
// Contiguous take the minimum and maximum over their blocks and hand the oldtype's sticky flags on
// (Indexed.java:110-177, Vector.java:99-135, Contiguous.java:71-98 — the three agree for the positive strides
// built here). Struct restates Struct.computeBounds (Struct.java:149-386) AS WRITTEN, in the order of the
// arrays: a component with ubSet REPLACES ub (the `if (max_ub > ub)` test is commented out at :243), one
// without moves ub whenever it reaches past every earlier unmarked component (trueUb, :251-258), even after a
// marker; lb mirrors it (:272-303). A marker is itself an unmarked component for the OTHER bound.
struct BoundsAcc {
  using i128 = __int128;
  bool strukt = false;
  bool any = false, have_tlb = false, have_tub = false, lbs = false, ubs = false;
  i128 lb = 0, ub = 0, tlb = 0, tub = 0;
  // `len` > 0 items of `old` (with data, or with a sticky flag), the first `st` base elements from the origin
  void add(i128 st, int64_t len, const TypeForm& old) {
    const i128 max_ub = st + (i128)(len - 1) * old.extent() + old.ub(), min_lb = st + old.lb();
    if (!strukt) {
      lb = any ? std::min(lb, min_lb) : min_lb;
      ub = any ? std::max(ub, max_ub) : max_ub;
      lbs = lbs || old.lb_set, ubs = ubs || old.ub_set;
      any = true;
      return;
    }
    any = true;
    if (old.ub_set) {
      ubs = true;
      ub = max_ub;
    } else if (!have_tub || max_ub > tub) {
      have_tub = true;
      tub = max_ub;
      ub = std::max(max_ub, st);
    }
    if (old.lb_set) {
      lbs = true;
      lb = min_lb;
    } else if (!have_tlb || min_lb < tlb) {
      have_tlb = true;
      tlb = min_lb;
      lb = std::min(min_lb, st);
    }
  }
};

// n blocks: block i is bl(i) items of oldf(i), one extent of that type apart, starting start(i) base elements
// from the origin. `proto` gives the new type's base element; `strukt` selects Struct's bounds rules.
template <class BL, class ST, class OF>
inline int flatten_form(int64_t n, BL bl, ST start, OF oldf, const TypeForm& proto, bool strukt, TypeForm* out,
                        std::string* err) {
  using i128 = __int128;
  const i128 lim = kMoveMaxBytes / proto.bsz;
  std::vector<ElemBlock> v;
  i128 size = 0;
  BoundsAcc acc;
  acc.strukt = strukt;
  for (int64_t i = 0; i < n; i++)
    if (bl(i) < 0) {
      *err = "negative blocklength " + std::to_string(bl(i)) + " at index " + std::to_string(i);
      return kTypeErrArg;
    }
  for (int64_t i = 0; i < n; i++) {
    const TypeForm& old = oldf(i);
    const int64_t len = bl(i);
    const int64_t onb = form_nblocks(old), osz = old.size(), oext = old.extent();
    if (len == 0 || (osz == 0 && !old.lb_set && !old.ub_set)) continue;
    const i128 st = start(i);
    if (st < 0 && osz != 0) {
      *err = "a negative displacement (" + std::to_string((long long)st) + " base elements at index " +
             std::to_string(i) + ") is not supported";
      return kTypeErrUnsupported;
    }
    const i128 hi = st + (i128)(len - 1) * oext + std::max(old.ub(), old.true_ub());
    size += (i128)len * osz;
    if (st > lim || st < -lim || hi > lim || size > lim || old.lb() < -lim) {
      *err = "block " + std::to_string(i) + " (length " + std::to_string(len) + ") reaches beyond 2^62 bytes";
      return kTypeErrArg;
    }
    acc.add(st, len, old);
    if (osz == 0) continue;  // a marker, or a type of markers only: bounds, no data
    auto push = [&](int64_t off, int64_t l) {
      if (!v.empty() && v.back().off + v.back().len == off) {
        v.back().len += l;
        return true;
      }
      if ((int64_t)v.size() >= kIndexedMaxBlocks) return false;
      v.push_back(ElemBlock{off, l});
      return true;
    };
    bool fits = true;
    int64_t o0, l0;
    form_block(old, 0, &o0, &l0);
    if (onb == 1 && oext == l0) {  // one block per item of old and the items abut: the run is one block
      fits = push((int64_t)st + o0, len * l0);
    } else {  // every item adds at least one merged block: the loop ends at the bound
      for (int64_t j = 0; j < len && fits; j++)
        for (int64_t b = 0; b < onb && fits; b++) {
          int64_t o, l;
          form_block(old, b, &o, &l);
          fits = push((int64_t)st + j * oext + o, l);
        }
    }
    if (!fits) {
      *err = "more than " + std::to_string(kIndexedMaxBlocks) + " blocks after merging (at index " + std::to_string(i) +
             ") are not supported";
      return kTypeErrUnsupported;
    }
  }
  if (acc.ub < acc.lb) {
    *err = "an explicit extent below 0 (lb " + std::to_string((long long)acc.lb) + ", ub " +
           std::to_string((long long)acc.ub) + ": extent " + std::to_string((long long)(acc.ub - acc.lb)) +
           ") is not supported";
    return kTypeErrUnsupported;
  }
  normal_form(proto, v, (int64_t)acc.lb, (int64_t)acc.ub, acc.lbs, acc.ubs, out);
  return kTypeOk;
}

template <class BL, class ST>
inline int irregular_form(int64_t n, BL bl, ST start, const TypeForm& old, TypeForm* out, std::string* err) {
  return flatten_form(n, bl, start, [&](int64_t) -> const TypeForm& { return old; }, old, false, out, err);
}

inline int indexed_args(int64_t n, const int64_t* bl, const int64_t* disp, std::string* err) {
  if (n < 0) {
    *err = "negative n " + std::to_string(n);
    return kTypeErrArg;
  }
  if (n > 0 && (!bl || !disp)) {
    *err = std::string("NULL ") + (!bl ? "blocklengths" : "displacements") + " with n = " + std::to_string(n);
    return kTypeErrArg;
  }
  return kTypeOk;
}

// Indexed(bl[], disp[], old): displacements in units of old's extent (Indexed.java)
inline int indexed_form(int64_t n, const int64_t* bl, const int64_t* disp, const TypeForm& old, TypeForm* out,
                        std::string* err) {
  const int rc = indexed_args(n, bl, disp, err);
  if (rc != kTypeOk) return rc;
  const int64_t oext = old.extent();
  return irregular_form(n, [&](int64_t i) { return bl[i]; }, [&](int64_t i) { return (__int128)disp[i] * oext; }, old,
                        out, err);
}

// Hindexed: displacements in base elements (mpiJava's "H" units are buffer indices, not bytes)
inline int hindexed_form(int64_t n, const int64_t* bl, const int64_t* disp, const TypeForm& old, TypeForm* out,
                         std::string* err) {
  const int rc = indexed_args(n, bl, disp, err);
  if (rc != kTypeOk) return rc;
  return irregular_form(n, [&](int64_t i) { return bl[i]; }, [&](int64_t i) { return (__int128)disp[i]; }, old, out, err);
}

// Hvector(count, bl, stride, old): block j starts j * stride base elements from the origin
inline int hvector_form(int64_t count, int64_t blocklength, int64_t stride, const TypeForm& old, TypeForm* out,
                        std::string* err) {
  if (count < 0 || blocklength < 0) {
    *err = std::string("negative ") + (count < 0 ? "count " + std::to_string(count) : "blocklength " + std::to_string(blocklength));
    return kTypeErrArg;
  }
  if (count > 1 && stride < 1) {
    *err = "stride " + std::to_string(stride) + " (below 1 with count " + std::to_string(count) + ") is not supported";
    return kTypeErrUnsupported;
  }
  if (blocklength == 0 || old.size() == 0) count = 0;
  if (count > 1) {  // settle the sizes before walking `count` blocks
    const __int128 lim = kMoveMaxBytes / old.bsz;
    const __int128 last = (__int128)(count - 1) * stride + (__int128)(blocklength - 1) * old.extent() + old.ub();
    if (last > lim || (__int128)count * blocklength > lim / old.size()) {
      *err = "count " + std::to_string(count) + " at stride " + std::to_string(stride) + " reaches beyond 2^62 bytes";
      return kTypeErrArg;
    }
    if (form_nblocks(old) == 1 && stride == blocklength * old.extent()) {  // the blocks abut: one run
      const int64_t run = count * blocklength;
      return irregular_form(1, [&](int64_t) { return run; }, [&](int64_t) { return (__int128)0; }, old, out, err);
    }
    if (count > kIndexedMaxBlocks) {  // no two of them merge
      *err = "count " + std::to_string(count) + " gives more than " + std::to_string(kIndexedMaxBlocks) +
             " blocks after merging, which is not supported";
      return kTypeErrUnsupported;
    }
  }
  return irregular_form(count, [&](int64_t) { return blocklength; }, [&](int64_t j) { return (__int128)j * stride; }, old,
                        out, err);
}

// Vector and Contiguous of any oldtype. An oldtype with explicit bounds (its extent is not its blocks' span) makes
// layouts the regular planner of mpjx_strided_plan.hpp cannot express, a Vector of a resized element for one: it
// is flattened here, as the Hvector of stride * old.extent; the result is regular again where its blocks are.
// Every other oldtype keeps vector_form, its limits included.
inline int vector_any_form(int64_t count, int64_t blocklength, int64_t stride, const TypeForm& old, TypeForm* out,
                           std::string* err) {
  if (!old.bounds) return vector_form(count, blocklength, stride, old, out, err);
  if (count < 0 || blocklength < 0) {
    *err = std::string("negative ") + (count < 0 ? "count" : "blocklength");
    return kTypeErrArg;
  }
  const __int128 hs = (__int128)stride * old.extent();
  if (hs > kMoveMaxBytes || hs < -kMoveMaxBytes) {
    *err = "count or stride too large";
    return kTypeErrArg;
  }
  return hvector_form(count, blocklength, (int64_t)hs, old, out, err);
}
inline int contiguous_any_form(int64_t count, const TypeForm& old, TypeForm* out, std::string* err) {
  if (!old.bounds) return contiguous_of(count, old, out, err);
  if (count < 0) {
    *err = "negative count";
    return kTypeErrArg;
  }
  // Contiguous.java:77-98: lb = old.lb, ub = lb + count * old.extent, which is the one block of `count` items
  return irregular_form(count > 0 ? 1 : 0, [&](int64_t) { return count; }, [&](int64_t) { return (__int128)0; }, old,
                        out, err);
}

// Struct(bl[], disp[], types[]): block i is bl[i] items of comp[i], one extent of that type apart, starting
// disp[i] BASE elements from the origin, packed in the order of the arrays (Struct.StructPacker.pack,
// Struct.java:448-464). A marker (MPJX_LB, MPJX_UB) has no base type and no data; every other component must
// have the one base type (Struct.java:100-117). The bounds are BoundsAcc's Struct rules.
inline int struct_form(int64_t n, const int64_t* bl, const int64_t* disp, const std::vector<TypeForm>& comp,
                       TypeForm* out, std::string* err) {
  const int rc = indexed_args(n, bl, disp, err);
  if (rc != kTypeOk) return rc;
  TypeForm proto = contiguous_form(0, 1, 0);
  bool pair = true;
  for (int64_t i = 0; i < n; i++) {
    const TypeForm& c = comp[(size_t)i];
    if (c.marker()) continue;
    if (proto.base == 0) proto.base = c.base, proto.bsz = c.bsz;
    else if (proto.base != c.base) {
      *err = "Base types of all component types in a Struct must agree (base type " + std::to_string(proto.base) +
             ", then " + std::to_string(c.base) + " at index " + std::to_string(i) + ")";
      return kTypeErrArg;
    }
    pair = pair && c.pair;
  }
  const int frc = flatten_form(n, [&](int64_t i) { return bl[i]; }, [&](int64_t i) { return (__int128)disp[i]; },
                               [&](int64_t i) -> const TypeForm& { return comp[(size_t)i]; }, proto, true, out, err);
  if (frc == kTypeOk) out->pair = pair && proto.base != 0;
  return frc;
}

// ---- the descriptor the kernel reads --------------------------------------------------------------------------

// One side of a segment. tab == nullptr: regular, `r` is k_strided's side. Otherwise irregular: r.base the
// origin of item 0, r.eb the item extent in bytes, r.bbg the granules per ITEM, r.nb.d the block count and
// tab the device table; r.sb is unused.
struct IndexedSide {
  StridedSide r;
  const IdxEnt* tab;
};

struct IndexedSeg {
  IndexedSide s, d;
  uint32_t ngran;  // granules of the packed stream (>= 1)
  uint32_t glog;   // log2 of the granule: 0..4
};

// Entry i of a table. On the device one 16-B load through a global-address-space pointer.
MPJX_HD inline IdxEnt idx_entry(const IdxEnt* tab, uint32_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
  typedef __attribute__((address_space(1))) const u64x2 G;
  const u64x2 v = ((G*)tab)[i];
  return IdxEnt{(int64_t)v.x, (uint64_t)v.y};
#else
  return tab[i];
#endif
}

// The block holding packed byte r of an item: the last of `n` entries whose prefix is <= r (pre[0] = 0).
// `entry(i)` reads entry i: from the device table, or from a copy of it.
template <class E>
MPJX_HD inline IdxEnt idx_search(E entry, uint32_t n, uint64_t r) {
  uint32_t lo = 0, hi = n;
  IdxEnt at = entry(0);
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    const IdxEnt e = entry(mid);
    if (e.pre <= r) lo = mid, at = e;
    else hi = mid;
  }
  return at;
}

// The byte address of packed granule q on an irregular side, its table read through `entry`: the item is
// q / gpi (FastDiv), the block comes from the search of the remainder's packed byte.
template <class E>
MPJX_HD inline uint64_t irregular_addr(const IndexedSide& x, uint32_t q, uint32_t glog, E entry) {
  const uint32_t k = fd_div(x.r.bbg, q);
  const uint64_t r = (uint64_t)(q - k * x.r.bbg.d) << glog;
  const IdxEnt e = idx_search(entry, x.r.nb.d, r);
  return x.r.base + (uint64_t)k * x.r.eb + (uint64_t)e.off + (r - e.pre);
}

// The byte address of packed granule q on one side (the table searched where it lies, in device memory)
MPJX_HD inline uint64_t indexed_addr(const IndexedSide& x, uint32_t q, uint32_t glog) {
  if (!x.tab) return strided_addr(x.r, q, glog);
  const IdxEnt* tab = x.tab;
  return irregular_addr(x, q, glog, [tab](uint32_t i) { return idx_entry(tab, i); });
}

// The kernel's descriptor of the move s -> d (equal non-zero totals); stab / dtab are the DEVICE tables of the
// irregular sides (ignored for a regular one). The granule is strided_granule_log's: an irregular side gives
// its every block offset and length and its extent (IrrLayout::amask, made once per type), so no access is
// misaligned and none straddles a block. kTypeErrUnsupported with *err set for a segment of more than
// kStridedMaxGran granules.
inline int plan_indexed_seg(const SideBytes& s, const IdxEnt* stab, const SideBytes& d, const IdxEnt* dtab,
                            IndexedSeg* out, std::string* err) {
  const uint32_t g = strided_granule_log(s, d);
  const int64_t ngran = s.total() >> g;
  if (ngran > kStridedMaxGran) {
    *err = "an indexed segment of " + std::to_string(s.total()) + " bytes in granules of " + std::to_string(1 << g) +
           " B exceeds 2^32 - 1 granules";
    return kTypeErrUnsupported;
  }
  auto side = [&](const SideBytes& x, const IdxEnt* tab) {
    IndexedSide y;
    y.tab = x.irr ? tab : nullptr;
    y.r.base = x.base;
    y.r.sb = (uint64_t)x.sb;
    y.r.eb = (uint64_t)x.eb;
    // an item's packed bytes are at most the segment's: below 2^32 granules
    y.r.bbg = fast_div((uint32_t)((x.irr ? x.irr->size : x.bb) >> g));
    y.r.nb = fast_div((uint32_t)std::min<int64_t>(x.nb, kStridedMaxGran));
    return y;
  };
  out->s = side(s, stab);
  out->d = side(d, dtab);
  out->ngran = (uint32_t)ngran;
  out->glog = g;
  return kTypeOk;
}

// ---- launch tables ------------------------------------------------------------------------------------------------

constexpr int kIndexedMax = 24;  // segments per launch table (the table is a kernel argument: 4 KiB at most)

struct IndexedTable {
  IndexedSeg seg[kIndexedMax];
  uint32_t tile0[kIndexedMax + 1];  // tile0[c] = first block of segment c; tile0[n] = the grid
  int n = 0;
};
static_assert(sizeof(IndexedTable) <= 4096, "the table is a kernel argument");

// As plan_strided_tables (the tiles are k_strided's: kStridedTile, kStridedTileNT)
inline void plan_indexed_tables(const std::vector<IndexedSeg>& segs, int64_t gran, std::vector<IndexedTable>* out,
                                int64_t max_tiles = kMoveMaxTiles) {
  out->clear();
  IndexedTable t;
  t.tile0[0] = 0;
  auto close = [&] {
    if (t.n > 0) out->push_back(t);
    t.n = 0;
    t.tile0[0] = 0;
  };
  for (const IndexedSeg& s : segs) {
    if (s.ngran == 0) continue;
    const int64_t tiles = strided_tiles(s.ngran, gran);
    if (t.n == kIndexedMax || (int64_t)t.tile0[t.n] + tiles > max_tiles) close();
    t.seg[t.n] = s;
    t.tile0[t.n + 1] = t.tile0[t.n] + (uint32_t)tiles;
    t.n++;
  }
  close();
}

}  // namespace mpjx
