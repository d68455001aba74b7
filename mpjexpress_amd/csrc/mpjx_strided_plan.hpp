// mpjx_strided_plan.hpp — derived datatypes (Contiguous, Vector) and the host-side planning of the strided
// block moves (mpjx_alltoallv_dt), with the geometry of k_strided (mpjx_k_strided.hip). No HIP include:
// plain C++17, compiled, tested and sanitized on the CPU (tests/cpp/strided_plan_test.cpp,
// tests/cpp/type_registry_test.cpp); the kernel includes the same header, so the mapping the test walks is
// the mapping the kernel runs.
//
// A datatype normalises to `nblocks` blocks of `blocklen` base elements, `stride` base elements apart
// (TypeForm). A message of `count` items of a type is, per side, a regular two-level layout in bytes
// (SideBytes): item k at base + k * eb, its block b at + b * sb, bb bytes each. The PACKED form of a
// message is its blocks in order; a move stores the packed bytes of the source layout in order into the
// destination layout, so the two block shapes need not agree. The irregular types (Hvector, Indexed, Hindexed:
// mpjx_indexed_plan.hpp) keep a block list instead (IrrLayout); TypeForm and SideBytes carry either kind, and
// the overlap checks below expand both.
//   granule  the largest power of two <= 16 B that divides both sides' block bytes, strides, extents and
//            base addresses: every block of either side starts and ends on a granule of the packed stream,
//            and every access of one granule is naturally aligned.
//   tile     `gran` consecutive granules of a segment's packed stream; lane t of a tile takes granule
//            x * gran + t (+ u * lanes), so neighbouring lanes take neighbouring granules of a block.
// Packed granule q of a segment lies in block q / bbg of its side (bbg = granules per block), at granule
// q % bbg of it; that block is block (q / bbg) % nb of item (q / bbg) / nb. All four numbers are below 2^32
// (plan_strided_seg rejects a segment of 2^32 granules or more), and the two divisors are fixed per segment,
// so the kernel divides by multiplying with a reciprocal the host computed (FastDiv).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "mpjx_moves_plan.hpp"

namespace mpjx {

// ---- datatypes: the normal form and the registry ---------------------------------------------------------

constexpr int kTypeOk = 0, kTypeErrArg = -1, kTypeErrUnsupported = -6;  // MPJX_SUCCESS / _ERR_ARG / _ERR_UNSUPPORTED
constexpr int kDerivedBase = 0x10000;                                   // the first derived handle

// One block of an irregular layout, in BYTES: where it starts from the item's origin, and how many packed
// bytes of the item precede it. The kernel's device table is an array of these (16 B each).
struct IdxEnt {
  int64_t off;
  uint64_t pre;
};

// The irregular form (Hvector, Indexed, Hindexed: mpjx_indexed_plan.hpp): the merged, non-empty blocks of one
// item in PACK order (the order of the constructor's arrays, not address order), in bytes. Immutable once
// made and shared by value-copies of the form, by every layout planned from it and by the communicators'
// device-table caches, so a call in flight keeps it alive after mpjx_type_free.
struct IrrLayout {
  std::vector<IdxEnt> tab;   // never empty; one block is irregular only for its offset (lb > 0)
  int64_t size = 0;          // packed bytes per item
  int64_t lb = 0, ub = 0;    // lowest byte and one past the highest byte of an item, from its origin
  uint64_t amask = 0;        // OR of every block's offset and length and of the extent: the type's part of the granule
  bool self_overlap = false; // two blocks of one item share a byte: legal to send, MPJX_ERR_ARG to receive into
  int64_t len(size_t b) const { return (int64_t)((b + 1 < tab.size() ? tab[b + 1].pre : (uint64_t)size) - tab[b].pre); }
};

// In elements of the base type. Regular (irr == nullptr): nblocks x blocklen at one stride, data from 0; contiguous
// types (nblocks <= 1) have stride == blocklen. Irregular: irr holds the blocks; nblocks/blocklen/stride are 0.
// The bounds are the blocks' own (lb = the lowest element, ub = one past the highest) unless `bounds` is set:
// then xlb / xub are the reference's lb and ub (an LB or UB marker of a Struct, or a type made from one that has
// them), lb_set / ub_set its sticky flags, and extent() = xub - xlb is any value >= 0, whatever the blocks
// span. Item k of a message still starts k * extent() after the origin and lb is not subtracted.
struct TypeForm {
  int base = 0;      // basic code 1..8 (0: a marker, or a Struct of markers only)
  int bsz = 0;       // bytes per base element
  int64_t nblocks = 0, blocklen = 0, stride = 0;
  std::shared_ptr<const IrrLayout> irr;
  int code = 0;      // the code the form was looked up by (type_form); keys the device-table caches
  bool pair = false; // made of (value, index) pair items: what MAXLOC / MINLOC reduce (the type constructors of
                     // mpjx_core.hip hand it on from the oldtype; the moves do not read it)
  bool bounds = false, lb_set = false, ub_set = false;
  int64_t xlb = 0, xub = 0;
  int64_t size() const { return irr ? irr->size / bsz : nblocks * blocklen; }
  // the lowest element and one past the highest element of one item's data, from its origin
  int64_t true_lb() const { return irr ? irr->lb / bsz : 0; }
  int64_t true_ub() const { return irr ? irr->ub / bsz : nblocks > 0 ? (nblocks - 1) * stride + blocklen : 0; }
  int64_t lb() const { return bounds ? xlb : true_lb(); }
  int64_t ub() const { return bounds ? xub : true_ub(); }
  int64_t extent() const { return ub() - lb(); }
  bool contiguous() const { return !irr && nblocks <= 1; }
  int64_t merged_blocks() const { return irr ? (int64_t)irr->tab.size() : nblocks; }
  bool marker() const { return base == 0; }
  // The reference's bounds: kept apart only where they are not the blocks' own, so that every type the five
  // older constructors make from basic types is the form it always was
  void set_bounds(int64_t lb, int64_t ub, bool lbs, bool ubs) {
    bounds = lbs || ubs || lb != true_lb() || ub != true_ub();
    lb_set = lbs, ub_set = ubs;
    xlb = bounds ? lb : 0, xub = bounds ? ub : 0;
  }
};

inline TypeForm contiguous_form(int base, int bsz, int64_t n) {
  TypeForm f;
  f.base = base;
  f.bsz = bsz;
  if (n > 0) f.nblocks = 1, f.blocklen = n, f.stride = n;
  return f;
}

constexpr int kCodeLB = 10, kCodeUB = 11;  // MPJX_LB / MPJX_UB (Datatype.java:68-69)

// The form of a basic code (1..8), a pair code (0x100 | base, base in {3, 5, 6, 7, 8}) or a marker (LB, UB: no
// base type, size 0, lb = ub = 0 with lbSet or ubSet, BasicType.java:145-170); false if none of them.
inline bool basic_form(int code, TypeForm* out) {
  static const int bytes[9] = {0, 1, 2, 2, 1, 4, 8, 4, 8};  // BYTE CHAR SHORT BOOLEAN INT LONG FLOAT DOUBLE
  if (code >= 1 && code <= 8) {
    *out = contiguous_form(code, bytes[code], 1);
    return true;
  }
  if (code == kCodeLB || code == kCodeUB) {
    *out = contiguous_form(0, 1, 0);
    out->set_bounds(0, 0, code == kCodeLB, code == kCodeUB);
    return true;
  }
  const int b = code & 0xff;
  if ((code & ~0xff) == 0x100 && (b == 3 || (b >= 5 && b <= 8))) {
    *out = contiguous_form(b, bytes[b], 2);
    out->pair = true;
    return true;
  }
  return false;
}

// Vector(count, blocklength, stride, old): blocklength and stride in items of `old` (Vector.java). `old` must
// be contiguous; count <= 1, an empty block and stride == blocklength normalise to contiguous.
inline int vector_form(int64_t count, int64_t blocklength, int64_t stride, const TypeForm& old, TypeForm* out,
                       std::string* err) {
  if (count < 0 || blocklength < 0) {
    *err = std::string("negative ") + (count < 0 ? "count" : "blocklength");
    return kTypeErrArg;
  }
  if (old.irr) {
    *err = "an irregular oldtype (" + std::to_string(old.irr->tab.size()) + " blocks) is not supported";
    return kTypeErrUnsupported;
  }
  if (!old.contiguous()) {
    *err = "a strided oldtype (" + std::to_string(old.nblocks) + " blocks of " + std::to_string(old.blocklen) +
           " at stride " + std::to_string(old.stride) + ") is not supported";
    return kTypeErrUnsupported;
  }
  const int64_t osz = old.size();
  const int64_t lim = kMoveMaxBytes / old.bsz;
  if (osz > 0 && blocklength > lim / osz) {
    *err = "blocklength too large";
    return kTypeErrArg;
  }
  const int64_t bl = blocklength * osz;  // base elements per block
  if (count == 0 || bl == 0) {
    *out = contiguous_form(old.base, old.bsz, 0);
    return kTypeOk;
  }
  if (count == 1 || stride == blocklength) {
    if (count > lim / bl) {
      *err = "count too large";
      return kTypeErrArg;
    }
    *out = contiguous_form(old.base, old.bsz, count * bl);
    return kTypeOk;
  }
  if (stride < blocklength) {
    *err = "stride " + std::to_string(stride) + " smaller than blocklength " + std::to_string(blocklength) +
           " (negative, zero or overlapping) is not supported";
    return kTypeErrUnsupported;
  }
  if (stride > lim / osz || count > lim / (stride * osz)) {
    *err = "count or stride too large";
    return kTypeErrArg;
  }
  out->base = old.base;
  out->bsz = old.bsz;
  out->nblocks = count;
  out->blocklen = bl;
  out->stride = stride * osz;
  return kTypeOk;
}

inline int contiguous_of(int64_t count, const TypeForm& old, TypeForm* out, std::string* err) {
  return vector_form(count < 0 ? count : (count > 0 ? 1 : 0), count, count, old, out, err);
}

// Process-wide, thread-safe: rank threads create and free types concurrently. Handles count up from
// kDerivedBase and are never reissued; a freed or unknown handle is not found.
class TypeRegistry {
 public:
  static TypeRegistry& get() {
    static TypeRegistry r;
    return r;
  }
  int add(const TypeForm& f) {
    std::lock_guard<std::mutex> g(mu_);
    slots_.push_back(Slot{f, true});
    return kDerivedBase + (int)slots_.size() - 1;
  }
  bool find(int code, TypeForm* out) {
    std::lock_guard<std::mutex> g(mu_);
    const int64_t i = (int64_t)code - kDerivedBase;
    if (i < 0 || i >= (int64_t)slots_.size() || !slots_[(size_t)i].live) return false;
    *out = slots_[(size_t)i].form;
    return true;
  }
  bool release(int code) {
    std::lock_guard<std::mutex> g(mu_);
    const int64_t i = (int64_t)code - kDerivedBase;
    if (i < 0 || i >= (int64_t)slots_.size() || !slots_[(size_t)i].live) return false;
    slots_[(size_t)i].live = false;
    slots_[(size_t)i].form.irr.reset();  // calls in flight hold their own reference
    return true;
  }

 private:
  struct Slot {
    TypeForm form;
    bool live;
  };
  std::mutex mu_;
  std::vector<Slot> slots_;
};

// Basic, pair and live derived codes; the markers only where `markers` says so (a component of a Struct)
inline bool type_form(int code, TypeForm* out, bool markers = false) {
  if (!markers && (code == kCodeLB || code == kCodeUB)) return false;
  if (!(code >= kDerivedBase ? TypeRegistry::get().find(code, out) : basic_form(code, out))) return false;
  out->code = code;
  return true;
}

// ---- one side of one message, in bytes -------------------------------------------------------------------

// `items` items of a type at byte address `base`: item k at base + k * eb, block b of it at + b * sb, bb
// bytes per block. A contiguous run is ONE item of ONE block (bb = sb = eb = total). An irregular layout
// (irr != nullptr) has item k's block b at base + k * eb + irr->tab[b].off; bb = sb = 0 and nb is its block
// count. `base` is the item's ORIGIN: an irregular type's lb is not subtracted (GenericPacker).
struct SideBytes {
  uint64_t base = 0;
  int64_t bb = 0, sb = 0, nb = 0, eb = 0, items = 0;
  std::shared_ptr<const IrrLayout> irr;
  int code = 0;  // the irregular type's code
  int64_t total() const { return irr ? items * irr->size : items * nb * bb; }
  int64_t blocks() const { return items * nb; }
  bool contiguous() const { return !irr && items * nb <= 1; }
  bool regular() const { return !irr; }
  // The address of packed byte p (numpy-style indexing; the tests' reference for the kernel's mapping)
  uint64_t at(int64_t p) const {
    if (irr) {
      const int64_t k = p / irr->size;
      const uint64_t r = (uint64_t)(p % irr->size);
      size_t b = 0;
      while (b + 1 < irr->tab.size() && irr->tab[b + 1].pre <= r) b++;
      return base + (uint64_t)(k * eb + irr->tab[b].off) + (r - irr->tab[b].pre);
    }
    const int64_t blk = p / bb, w = p % bb;
    return base + (uint64_t)((blk / nb) * eb + (blk % nb) * sb + w);
  }
  // Consecutive items may share a byte: an item's blocks reach past the next item's origin (an explicit extent
  // below the blocks' span) and the cheap argument that they merely interleave — a regular side whose items all
  // fit before its second block, as the columns of a panel do — does not hold. Only the exact check can tell.
  bool items_may_overlap() const {
    if (items <= 1 || total() <= 0) return false;
    if (irr) return eb < irr->ub - irr->lb;
    if (eb >= (nb - 1) * sb + bb) return false;
    return !(eb >= bb && (items - 1) * eb + bb <= sb);
  }
  // First and one-past-last byte address touched (first == last when empty): the blocks' own bounds, whatever
  // the type's lb and ub say (eb >= 0, so the last item reaches highest)
  void span(uint64_t* lo, uint64_t* hi) const {
    *lo = *hi = base;
    if (total() <= 0) return;
    if (irr) {
      *lo = base + (uint64_t)irr->lb;
      *hi = base + (uint64_t)((items - 1) * eb + irr->ub);
    } else {
      *hi = base + (uint64_t)((items - 1) * eb + (nb - 1) * sb + bb);
    }
  }
};

// `count` items of `f` whose first base element is `disp` base elements past byte address `buf`. False with
// *err set for a negative count or displacement, or a layout beyond 2^62 bytes.
inline bool plan_side(const TypeForm& f, uint64_t buf, int64_t count, int64_t disp, SideBytes* out, std::string* err,
                      const char* what = "count") {
  *out = SideBytes{};
  if (count < 0 || disp < 0) {
    *err = std::string("negative ") + (count < 0 ? what : "displacement");
    return false;
  }
  const int64_t lim = kMoveMaxBytes / f.bsz;
  if (disp > lim) {
    *err = "displacement too large";
    return false;
  }
  out->base = buf + (uint64_t)(disp * f.bsz);
  if (count == 0 || f.size() == 0) return true;
  // the last item's highest element, (count - 1) * extent + true_ub, stays within the limit (true_ub <= lim
  // by construction; extent 0 puts every item at the same place)
  const int64_t ext = f.extent();
  if (ext > 0 && count - 1 > (lim - f.true_ub()) / ext) {
    *err = std::string(what) + " too large";
    return false;
  }
  if (count > lim / f.size()) {
    *err = std::string(what) + " too large";
    return false;
  }
  const bool abut = ext == f.size();  // consecutive items of a one-block type form one run
  if (f.irr && f.irr->tab.size() == 1 && (abut || count == 1)) {  // one block lb elements in
    out->base += (uint64_t)f.irr->tab[0].off;
    out->bb = out->sb = out->eb = count * f.irr->size;
    out->nb = out->items = 1;
  } else if (f.irr) {
    out->irr = f.irr;
    out->code = f.code;
    out->nb = (int64_t)f.irr->tab.size();
    out->eb = ext * f.bsz;
    out->items = count;
  } else if ((f.contiguous() && abut) || count * f.nblocks == 1) {
    out->bb = out->sb = out->eb = count * f.size() * f.bsz;
    out->nb = out->items = 1;
  } else {
    out->bb = f.blocklen * f.bsz;
    out->sb = f.stride * f.bsz;
    out->nb = f.nblocks;
    out->eb = f.extent() * f.bsz;
    out->items = count;
  }
  return true;
}

// ---- division by a per-segment constant -------------------------------------------------------------------

// n / d for n, d < 2^32, d >= 1, as the high 64 bits of m * n with m = floor((2^64 - 1) / d) + 1 (exact for
// every 32-bit n: Lemire, Kaser, Kurz, "Faster remainder by direct computation", 2019). d = 1 has no such m
// in 64 bits: m = 0 stands for it.
struct FastDiv {
  uint64_t m = 0;
  uint32_t d = 1;
};
inline FastDiv fast_div(uint32_t d) {
  FastDiv f;
  f.d = d;
  f.m = d > 1 ? ~(uint64_t)0 / d + 1 : 0;
  return f;
}
MPJX_HD inline uint32_t fd_div(const FastDiv& f, uint32_t n) {
  if (f.m == 0) return n;
#if defined(__HIP_DEVICE_COMPILE__)
  return (uint32_t)__umul64hi(f.m, (uint64_t)n);
#else
  return (uint32_t)(((unsigned __int128)f.m * n) >> 64);
#endif
}

// ---- the descriptor the kernel reads ------------------------------------------------------------------------

struct StridedSide {
  uint64_t base;  // byte address of item 0
  uint64_t sb, eb;  // stride and extent in bytes
  FastDiv bbg;    // granules per block
  FastDiv nb;     // blocks per item
};

struct StridedSeg {
  StridedSide s, d;
  uint32_t ngran;  // granules of the packed stream (>= 1)
  uint32_t glog;   // log2 of the granule: 0..4
};

// The byte address of packed granule q on one side
MPJX_HD inline uint64_t strided_addr(const StridedSide& x, uint32_t q, uint32_t glog) {
  const uint32_t blk = fd_div(x.bbg, q), w = q - blk * x.bbg.d;
  const uint32_t k = fd_div(x.nb, blk), b = blk - k * x.nb.d;
  return x.base + (uint64_t)k * x.eb + (uint64_t)b * x.sb + ((uint64_t)w << glog);
}

// log2 of the largest power of two <= 16 that divides both sides' block bytes, strides, extents and bases
inline uint64_t side_align_mask(const SideBytes& x) {
  return x.base | (uint64_t)x.eb | (x.irr ? x.irr->amask : (uint64_t)x.bb | (uint64_t)x.sb);
}
// (an irregular side gives its every block offset and length and its extent: mpjx_indexed_plan.hpp)
inline uint32_t strided_granule_log(const SideBytes& s, const SideBytes& d) {
  const uint64_t all = side_align_mask(s) | side_align_mask(d) | 16u;
  uint32_t g = 0;
  while (!((all >> g) & 1u)) g++;
  return g;
}

constexpr int64_t kStridedMaxGran = ((int64_t)1 << 32) - 1;  // granules per segment

// The kernel's descriptor of the move s -> d (equal non-zero totals). kTypeErrUnsupported with *err set for
// a segment of more than kStridedMaxGran granules.
inline int plan_strided_seg(const SideBytes& s, const SideBytes& d, StridedSeg* out, std::string* err) {
  const uint32_t g = strided_granule_log(s, d);
  const int64_t ngran = s.total() >> g;
  if (ngran > kStridedMaxGran) {
    *err = "a strided segment of " + std::to_string(s.total()) + " bytes in granules of " + std::to_string(1 << g) +
           " B exceeds 2^32 - 1 granules";
    return kTypeErrUnsupported;
  }
  auto side = [&](const SideBytes& x) {
    StridedSide y;
    y.base = x.base;
    y.sb = (uint64_t)x.sb;
    y.eb = (uint64_t)x.eb;
    y.bbg = fast_div((uint32_t)(x.bb >> g));  // bb <= total: below 2^32 granules
    // more blocks per item than the segment has granules cannot be reached: any divisor above them will do
    y.nb = fast_div((uint32_t)std::min<int64_t>(x.nb, kStridedMaxGran));
    return y;
  };
  out->s = side(s);
  out->d = side(d);
  out->ngran = (uint32_t)ngran;
  out->glog = g;
  return kTypeOk;
}

// ---- tiles and launch tables --------------------------------------------------------------------------------

MPJX_HD inline int64_t strided_tiles(uint32_t ngran, int64_t gran) { return ((int64_t)ngran + gran - 1) / gran; }

// Granules per tile of the kernel's two forms, and the packed bytes per call from which it streams
// (non-temporal loads and stores): k_moves' shapes and threshold.
constexpr int64_t kStridedTile = 256 * 4, kStridedTileNT = 512 * 1;
constexpr int64_t kStridedStreamBytes = (int64_t)64 << 20;

constexpr int kStridedMax = 32;  // segments per launch table (the table is a kernel argument: 4 KiB at most)

struct StridedTable {
  StridedSeg seg[kStridedMax];
  uint32_t tile0[kStridedMax + 1];  // tile0[c] = first block of segment c; tile0[n] = the grid
  int n = 0;
};

// The launch tables of `segs` for tiles of `gran` granules, in order, as plan_tables makes them: a table is
// closed when it holds kStridedMax segments or max_tiles tiles (a segment has fewer than 2^32 / gran tiles, so
// none needs cutting while max_tiles * gran >= 2^32). Every table has n >= 1 and no empty segment.
inline void plan_strided_tables(const std::vector<StridedSeg>& segs, int64_t gran, std::vector<StridedTable>* out,
                                int64_t max_tiles = kMoveMaxTiles) {
  out->clear();
  StridedTable t;
  t.tile0[0] = 0;
  auto close = [&] {
    if (t.n > 0) out->push_back(t);
    t.n = 0;
    t.tile0[0] = 0;
  };
  for (const StridedSeg& s : segs) {
    if (s.ngran == 0) continue;
    const int64_t tiles = strided_tiles(s.ngran, gran);
    if (t.n == kStridedMax || (int64_t)t.tile0[t.n] + tiles > max_tiles) close();
    t.seg[t.n] = s;
    t.tile0[t.n + 1] = t.tile0[t.n] + (uint32_t)tiles;
    t.n++;
  }
  close();
}

// ---- exact overlap checks -------------------------------------------------------------------------------------

constexpr int64_t kOverlapMaxBlocks = 65536;  // beyond this many blocks in a call's tables the check is skipped

struct AddrBlock {
  uint64_t lo, hi;  // [lo, hi)
  int seg;
};

inline int64_t count_blocks(const std::vector<SideBytes>& v) {
  int64_t n = 0;
  for (const SideBytes& x : v) {
    if (x.total() <= 0) continue;
    if (x.blocks() > kOverlapMaxBlocks) return kOverlapMaxBlocks + 1;  // no sum can overflow
    n += x.blocks();
  }
  return n;
}

inline void expand_blocks(const std::vector<SideBytes>& v, std::vector<AddrBlock>* out) {
  out->clear();
  for (int j = 0; j < (int)v.size(); j++) {
    const SideBytes& x = v[(size_t)j];
    if (x.total() <= 0) continue;
    for (int64_t k = 0; k < x.items; k++)
      for (int64_t b = 0; b < x.nb; b++) {
        const uint64_t lo = x.base + (uint64_t)(k * x.eb + (x.irr ? x.irr->tab[(size_t)b].off : b * x.sb));
        out->push_back(AddrBlock{lo, lo + (uint64_t)(x.irr ? x.irr->len((size_t)b) : x.bb), j});
      }
  }
  std::sort(out->begin(), out->end(), [](const AddrBlock& a, const AddrBlock& b) { return a.lo < b.lo; });
}

enum OverlapResult { kNoOverlap = 0, kRecvOverlap = 1, kSendRecvOverlap = 2, kOverlapUnchecked = 3 };

// True if no receive layout's bounding span meets another receive layout's or a send layout's: then no two of
// them share a byte, whatever their blocks, and nothing needs expanding (the common call: one region per
// peer). Send layouts may share bytes with each other.
inline bool spans_disjoint(const std::vector<SideBytes>& S, const std::vector<SideBytes>& R) {
  struct Span {
    uint64_t lo, hi;
    bool recv;
  };
  std::vector<Span> v;
  for (int k = 0; k < 2; k++)
    for (const SideBytes& x : k ? R : S) {
      if (x.total() <= 0) continue;
      if (k == 1 && x.items_may_overlap()) return false;  // a receive layout that may overlap itself
      Span sp{0, 0, k == 1};
      x.span(&sp.lo, &sp.hi);
      v.push_back(sp);
    }
  std::sort(v.begin(), v.end(), [](const Span& a, const Span& b) { return a.lo < b.lo; });
  uint64_t send_hi = 0, recv_hi = 0;  // the furthest end among the spans before this one
  for (const Span& x : v) {
    if (x.lo < recv_hi || (x.recv && x.lo < send_hi)) return false;
    (x.recv ? recv_hi : send_hi) = std::max(x.recv ? recv_hi : send_hi, x.hi);
  }
  return true;
}

// Exact: two receive layouts that share a byte (*a, *b = their indices), or a send layout that shares a byte
// with a receive layout. Layouts whose bounding spans overlap but whose blocks interleave (two columns of
// one matrix) do not overlap. Disjoint spans are settled without expanding, at any size; otherwise
// kOverlapUnchecked when the tables hold more than kOverlapMaxBlocks blocks.
inline OverlapResult strided_overlap(const std::vector<SideBytes>& S, const std::vector<SideBytes>& R, int* a, int* b) {
  if (spans_disjoint(S, R)) return kNoOverlap;
  const int64_t ns = count_blocks(S), nr = count_blocks(R);
  if (ns + nr > kOverlapMaxBlocks) return kOverlapUnchecked;
  std::vector<AddrBlock> sb, rb;
  expand_blocks(S, &sb);
  expand_blocks(R, &rb);
  for (size_t k = 1; k < rb.size(); k++)
    if (rb[k - 1].hi > rb[k].lo) {
      *a = rb[k - 1].seg;
      *b = rb[k].seg;
      return kRecvOverlap;
    }
  // the receive blocks are disjoint and sorted: a merge finds any send block that meets one
  size_t i = 0;
  for (const AddrBlock& x : sb) {
    while (i < rb.size() && rb[i].hi <= x.lo) i++;
    if (i < rb.size() && rb[i].lo < x.hi) {
      *a = x.seg;
      *b = rb[i].seg;
      return kSendRecvOverlap;
    }
  }
  return kNoOverlap;
}

}  // namespace mpjx
