// mpjx_indexed_plan.hpp — the irregular derived datatypes (Hvector, Indexed, Hindexed) and the host-side
// planning of k_indexed (mpjx_k_indexed.hip). No HIP include: plain C++17, compiled, tested and sanitized on
// the CPU (tests/cpp/indexed_plan_test.cpp); the kernel includes the same header, so the address function the
// test walks is the one the kernel runs.
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

// The form of `blocks` (pack order, merged, none empty) with bounds lb, ub: regular where the list is.
inline void normal_form(const TypeForm& old, const std::vector<ElemBlock>& v, int64_t lb, int64_t ub, TypeForm* out) {
  *out = contiguous_form(old.base, old.bsz, 0);
  if (v.empty()) return;
  bool reg = v[0].off == 0;
  const int64_t st = v.size() > 1 ? v[1].off - v[0].off : v[0].len;
  for (size_t i = 1; reg && i < v.size(); i++) reg = v[i].len == v[0].len && v[i].off - v[i - 1].off == st;
  if (reg && st >= v[0].len) {
    out->nblocks = (int64_t)v.size();
    out->blocklen = v[0].len;
    out->stride = st;
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
}

// n blocks: block i is bl(i) items of `old`, old.extent apart, starting start(i) base elements from the
// origin.
template <class BL, class ST>
inline int irregular_form(int64_t n, BL bl, ST start, const TypeForm& old, TypeForm* out, std::string* err) {
  using i128 = __int128;
  const i128 lim = kMoveMaxBytes / old.bsz;
  const int64_t onb = form_nblocks(old), osz = old.size(), oext = old.extent();
  std::vector<ElemBlock> v;
  i128 size = 0, lb = 0, ub = 0;
  bool any = false;
  for (int64_t i = 0; i < n; i++)
    if (bl(i) < 0) {
      *err = "negative blocklength " + std::to_string(bl(i)) + " at index " + std::to_string(i);
      return kTypeErrArg;
    }
  for (int64_t i = 0; i < n; i++) {
    const int64_t len = bl(i);
    if (len == 0 || osz == 0) continue;
    const i128 st = start(i);
    if (st < 0) {
      *err = "a negative displacement (" + std::to_string((long long)st) + " base elements at index " +
             std::to_string(i) + ") is not supported";
      return kTypeErrUnsupported;
    }
    const i128 hi = st + (i128)(len - 1) * oext + old.ub();
    size += (i128)len * osz;
    if (st > lim || hi > lim || size > lim) {
      *err = "block " + std::to_string(i) + " (length " + std::to_string(len) + ") reaches beyond 2^62 bytes";
      return kTypeErrArg;
    }
    lb = any ? std::min(lb, st + old.lb()) : st + old.lb();
    ub = any ? std::max(ub, hi) : hi;
    any = true;
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
    if (onb == 1) {  // one block per item of old: its extent is its length, so the run is one block
      int64_t o, l;
      form_block(old, 0, &o, &l);
      fits = push((int64_t)st + o, len * l);
    } else {  // every item adds at least onb - 1 >= 1 merged blocks: the loop ends at the bound
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
  normal_form(old, v, (int64_t)lb, (int64_t)ub, out);
  return kTypeOk;
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
