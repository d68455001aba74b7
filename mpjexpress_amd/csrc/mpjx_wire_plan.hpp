// mpjx_wire_plan.hpp — the launch table and the per-lane arithmetic of k_wire (mpjx_k_wire.hip): the typed <->
// MPI.PACKED pairs of a claimed point-to-point batch, packed or unpacked on the fly in ONE launch per table. No
// HIP include: plain C++17, compiled, tested and sanitized on the CPU (tests/cpp/wire_plan_test.cpp); the kernel
// includes the same header, so the mapping the test walks is the mapping the kernel runs.
//
// A wire pair has a typed layout on one side and an mpjbuf image (mpjx_pack_plan.hpp: one section at position 0)
// on the other:
//   pack     typed send -> PACKED receive: the 8 header bytes of pack_header_word(base, words) at the image, then
//            the send layout's elements in pack order, each base word big-endian: what mpjx_pack(position 0) writes
//   unpack   PACKED send -> typed receive: the image's first section into the receive layout. The host knows only
//            the image's length: the kernel reads the count n from the header, checks it (wire_check_header) and
//            moves n words. n may end inside a granule: the granules wholly below n words move whole, the one that
//            n cuts is moved word by word by the lane that owns it, the ones above are not touched (wire_lane).
// A WireSeg is PackSeg's content plus the direction, the capacity in words, the bytes sent and the address of the
// 8-byte result slot {code, n} an unpack stores for the host. The granule is k_pack's (strided_granule_log over
// the layout and the payload at image + 8): it holds whole base words and never straddles a block on either side.
// The grid is the sum of the segments' tiles (tile0[], as k_msgs); a segment without payload still has one tile,
// so that its header is written or checked.
#pragma once
#include "mpjx_pack_plan.hpp"

namespace mpjx {

constexpr int kBasePacked = 9;  // MPI.PACKED's base type code (src/mpi/MPI.java:96, Datatype.java:67)
constexpr uint32_t kWirePack = 0, kWireUnpack = 1;
// the codes of a malformed header: MPJX_MPJBUF_BAD_TYPE / _BAD_COUNT / _OVERRUN
constexpr int kWireBadType = 1, kWireBadCount = 2, kWireOverrun = 3;

struct WireSeg {
  IndexedSide lay;  // the typed side's layout: item 0's origin, lb not subtracted
  uint64_t pay;     // byte address of the payload (image + 8)
  uint64_t hdr;     // byte address of the header (image)
  uint64_t header;  // pack: the header word to store
  int64_t cap;      // unpack: the receive layout's base elements
  int64_t sent;     // unpack: the bytes of the image that were sent (>= 8)
  uint64_t slot;    // unpack: byte address of the host-readable result slot {int32 code, int32 n}
  uint32_t ngran;   // granules of the packed stream the grid covers (0: header only)
  uint32_t glog;    // log2 of the granule: wlog..4
  uint32_t wlog;    // log2 of the base word: 0..3
  uint32_t lin;     // the typed side is one contiguous run: its address is linear too
  int code;         // the mpjbuf type code: base type code - 1
  uint32_t unpack;  // kWirePack / kWireUnpack
};

constexpr int kWireTableBytes = 4096;  // the table is a kernel argument
constexpr int kWireMax = (kWireTableBytes - 8) / (int)(sizeof(WireSeg) + sizeof(uint32_t));  // n and tile0's extra entry: 8 B

struct WireTable {
  WireSeg seg[kWireMax];
  uint32_t tile0[kWireMax + 1];  // tile0[c] = first block of segment c; tile0[n] = the grid
  int n = 0;
};
static_assert(sizeof(WireTable) <= kWireTableBytes, "the table is a kernel argument");
static_assert(kWireMax >= 16, "a WireSeg has grown beyond what a table is worth");

// typed send -> PACKED receive: `lay` is the send layout (`tab` its device table if irregular), `image` the
// receiver's image. The caller has checked 8 + lay.total() <= room, words <= kPackMaxWords and the alignments.
inline void plan_wire_pack(const SideBytes& lay, const IdxEnt* tab, uint64_t image, int base, int bsz, WireSeg* out) {
  PackSection sec;
  sec.h = 0;
  sec.pay = 8;
  sec.words = lay.total() / bsz;
  sec.end = 8 + lay.total();
  PackSeg p;
  plan_pack_seg(lay, tab, image, sec.end, sec, base, bsz, nullptr, &p);
  *out = WireSeg{};
  out->lay = p.lay;
  out->pay = p.pay;
  out->hdr = p.hdr;
  out->header = p.header;
  out->ngran = p.ngran;
  out->glog = p.glog;
  out->wlog = p.wlog;
  out->lin = p.lin;
  out->code = p.code;
  out->unpack = kWirePack;
}

// PACKED send -> typed receive: `lay` is the receive layout, `image` the sender's image of `sent` (>= 8) bytes,
// `slot` the result slot. The grid covers min(capacity, sent - 8) bytes of payload, the most a header that passes
// the kernel's checks can announce.
inline void plan_wire_unpack(const SideBytes& lay, const IdxEnt* tab, uint64_t image, int64_t sent, int base, int bsz,
                             uint64_t slot, WireSeg* out) {
  PackSection sec;
  sec.h = 0;
  sec.pay = 8;
  sec.words = lay.total() / bsz;
  sec.end = 8 + lay.total();
  PackSeg p;
  plan_pack_seg(lay, tab, image, sec.end, sec, base, bsz, nullptr, &p);
  *out = WireSeg{};
  out->lay = p.lay;
  out->pay = p.pay;
  out->hdr = p.hdr;
  out->cap = sec.words;
  out->sent = sent;
  out->slot = slot;
  out->glog = p.glog;
  out->wlog = p.wlog;
  out->lin = p.lin;
  out->code = p.code;
  out->unpack = kWireUnpack;
  const int64_t most = std::min<int64_t>(lay.total(), sent - 8);  // <= the layout's total: below 2^32 granules
  const int64_t gran = (int64_t)1 << p.glog;
  out->ngran = most > 0 ? (uint32_t)((most + gran - 1) >> p.glog) : 0u;
}

// The blocks segment `a` takes in a launch with tiles of `tile` granules: one at least
MPJX_HD inline int64_t wire_tiles(const WireSeg& a, int64_t tile) {
  const int64_t t = strided_tiles(a.ngran, tile);
  return t > 0 ? t : 1;
}

// The launch tables of `segs`, in order: a table is closed when it holds kWireMax segments or max_tiles tiles.
inline void plan_wire_tables(const std::vector<WireSeg>& segs, int64_t tile, std::vector<WireTable>* out,
                             int64_t max_tiles = kMoveMaxTiles) {
  out->clear();
  WireTable t;
  t.tile0[0] = 0;
  auto close = [&] {
    if (t.n > 0) out->push_back(t);
    t.n = 0;
    t.tile0[0] = 0;
  };
  for (const WireSeg& s : segs) {
    const int64_t tiles = wire_tiles(s, tile);
    if (t.n == kWireMax || (int64_t)t.tile0[t.n] + tiles > max_tiles) close();
    t.seg[t.n] = s;
    t.tile0[t.n + 1] = t.tile0[t.n] + (uint32_t)tiles;
    t.n++;
  }
  close();
}

// ---- what one lane does (shared by the kernel and the CPU walk) -------------------------------------------------

// The byte address of packed granule q on the typed side
MPJX_HD inline uint64_t wire_lay_addr(const WireSeg& a, uint32_t q) {
  if (a.lin) return a.lay.r.base + ((uint64_t)q << a.glog);
  return indexed_addr(a.lay, q, a.glog);
}

// The count field of the header word `hd` as a little-endian device loads it
MPJX_HD inline int64_t wire_header_count(uint64_t hd) {
  const uint32_t v = (uint32_t)(hd >> 32);
  const uint32_t n = (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24);
  return (int64_t)(int32_t)n;
}

// The checks of an unpack's header, in k_pack's order, before any payload byte is loaded: 0, or the code. *n is
// the count announced. A header that passes has 8 + n * w <= sent and n <= cap: every load and store is covered.
MPJX_HD inline int wire_check_header(const WireSeg& a, uint64_t hd, int64_t* n) {
  *n = wire_header_count(hd);
  if ((int)(hd & 0xffu) != a.code) return kWireBadType;
  if (*n < 0 || 8 + (*n << a.wlog) > a.sent) return kWireOverrun;
  if (*n > a.cap) return kWireBadCount;
  return 0;
}

// What the lane of packed granule q does in an unpack of n words: moves the granule whole, moves its first r
// words (the granule n cuts), or nothing
struct WireLane {
  bool whole;
  uint32_t r;
};
MPJX_HD inline WireLane wire_lane(const WireSeg& a, int64_t n, uint64_t q) {
  const uint64_t nb = (uint64_t)n << a.wlog;
  const uint64_t at = q << a.glog;
  WireLane l;
  l.whole = at + ((uint64_t)1 << a.glog) <= nb;
  l.r = !l.whole && at < nb ? (uint32_t)((nb - at) >> a.wlog) : 0u;
  return l;
}

// The 8 bytes of the result slot as one word: the code in the low half, n in the high half
MPJX_HD inline uint64_t wire_slot_word(int code, int64_t n) { return (uint64_t)(uint32_t)code | ((uint64_t)(uint32_t)n << 32); }

}  // namespace mpjx
