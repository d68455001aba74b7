// mpjx_transpose_plan.hpp — the eligibility test, descriptor and tile geometry of k_transpose
// (mpjx_k_transpose.hip): the element transpose among the strided moves. No HIP include: plain C++17, compiled,
// tested and sanitized on the CPU (tests/cpp/transpose_plan_test.cpp); the kernel includes the same header, so
// the mapping the test walks is the mapping the kernel runs.
//
// A type whose extent was resized to one element (a Struct with an UB marker) makes consecutive items
// consecutive elements: `count` items of a column type are `count` adjacent columns of a row-major matrix, and
// moving them to or from a contiguous run is a transpose. For k_strided's mapping that is the worst case: lanes
// that are neighbours in the packed stream touch addresses one row stride apart. k_transpose moves a tile
// through LDS instead, so that both global sides are accessed with consecutive lanes on consecutive granules.
//   X        the strided side: R = nb rows `sb` bytes apart, C = items columns one granule apart
//   Y        the contiguous side: packed granule q = c * R + r at ybase + q * g
//   tile     T x T granules, T = 64 for granules of 1, 2 and 4 bytes and 32 for 8 and 16 bytes: a tile row is
//            64 to 512 bytes of X; tile x of a segment is tile row x / ntc, tile column x % ntc (FastDiv)
//   lane     a workgroup of kTrLanes lanes walks the T * T slots of its tile twice: slot i as (i / T, i % T)
//            along X (neighbouring lanes on neighbouring columns) and as (i % T, i / T) along Y (neighbouring
//            lanes on neighbouring rows). The first walk loads its side and stores to LDS, the second loads
//            from LDS and stores to its side; gather (X -> Y) walks X first, scatter (Y -> X) walks Y first.
//   LDS      slot (a, b) of the FIRST walk at a * pitch + b * g bytes, pitch = T * g + max(g, 4): the first
//            walk's lanes store consecutive granules, the second walk's lanes read `pitch` bytes apart, which
//            is 17, 33, 65, 66 and 132 dwords for g = 1 .. 16: conflict-free by the bank rule of each load
//            (ds_read_u8/u16/b32 32 banks of 4 B per 32 lanes; ds_read_b64 64 banks per 32 lanes; ds_read_b128
//            64 banks per 16 lanes)
#pragma once
#include "mpjx_strided_plan.hpp"

namespace mpjx {

constexpr int kTrLanes = 256;

MPJX_HD inline uint32_t tr_tile_side(uint32_t glog) { return glog <= 2 ? 64u : 32u; }
MPJX_HD inline uint32_t tr_pitch(uint32_t glog) {
  return (tr_tile_side(glog) << glog) + ((1u << glog) > 4u ? (1u << glog) : 4u);
}
constexpr uint32_t kTrLdsBytes = 32 * (32 * 16 + 16);  // the largest tile: 16,896 B (64 * 260 = 16,640 for 4 B)

struct TransposeSeg {
  uint64_t xbase, ybase;  // byte addresses of X's granule (0, 0) and of Y's run
  uint64_t sb;            // X's row stride in bytes
  uint32_t R, C;          // rows (X.nb) and columns (X.items): R * C <= kStridedMaxGran granules
  FastDiv ntc;            // tile columns: ceil(C / T)
  uint32_t glog;          // log2 of the granule: 0..4
  uint32_t gather;        // 1: X -> Y (X is the source); 0: Y -> X
};

MPJX_HD inline uint64_t tr_addr_x(const TransposeSeg& t, uint32_t r, uint32_t c) {
  return t.xbase + (uint64_t)r * t.sb + ((uint64_t)c << t.glog);
}
MPJX_HD inline uint64_t tr_addr_y(const TransposeSeg& t, uint32_t r, uint32_t c) {
  return t.ybase + (((uint64_t)c * t.R + r) << t.glog);
}

// Slot i (0 .. T * T) of tile x on one walk
struct TrSlot {
  uint32_t r, c;    // the granule's row and column in X
  uint32_t a, b;    // its row and column in the tile
  bool on;          // inside the R x C granules: a predicated-off lane loads and stores nothing
};
MPJX_HD inline TrSlot tr_slot(const TransposeSeg& t, uint32_t x, uint32_t i, bool along_x) {
  const uint32_t T = tr_tile_side(t.glog), tlog = T == 64 ? 6 : 5;
  const uint32_t ty = fd_div(t.ntc, x), tx = x - ty * t.ntc.d;
  const uint32_t hi = i >> tlog, lo = i & (T - 1);
  TrSlot s;
  s.a = along_x ? hi : lo;
  s.b = along_x ? lo : hi;
  // ty < ceil(R / T) and tx < ceil(C / T): the products stay below 2^32 + T, computed in 64 bits
  const uint64_t r = (uint64_t)ty * T + s.a, c = (uint64_t)tx * T + s.b;
  s.on = r < t.R && c < t.C;
  s.r = (uint32_t)r;
  s.c = (uint32_t)c;
  return s;
}
// The LDS byte offset of tile slot (a, b) for the walk that goes FIRST (see the header comment)
MPJX_HD inline uint32_t tr_lds(const TransposeSeg& t, const TrSlot& s) {
  const bool x_first = t.gather != 0;
  return (x_first ? s.a : s.b) * tr_pitch(t.glog) + ((x_first ? s.b : s.a) << t.glog);
}

inline int64_t tr_tiles(const TransposeSeg& t) {
  const int64_t T = tr_tile_side(t.glog);
  return (((int64_t)t.R + T - 1) / T) * (int64_t)t.ntc.d;
}

// MPJX_TRANSPOSE=0 (read per call by the dispatcher) sends every segment back to k_strided.
//
// The eligibility of the move s -> d: both sides regular, exactly one of them (X) one granule per block
// (bb == granule), its consecutive items consecutive granules (eb == bb), nb >= 2 and items >= 2, and the other
// (Y) one contiguous run. The granule is strided_granule_log's, so elements of 1, 2, 4, 8 and 16 bytes
// qualify and wider blocks keep k_strided, which is coalesced from 64-B blocks up. No further threshold (a
// minimum for min(R, C), say) is set: none has been measured.
inline bool transpose_side(const SideBytes& x, const SideBytes& y, uint32_t g) {
  return x.regular() && y.contiguous() && x.bb == ((int64_t)1 << g) && x.eb == x.bb && x.nb >= 2 && x.items >= 2;
}
inline bool plan_transpose_seg(const SideBytes& s, const SideBytes& d, TransposeSeg* out) {
  if (!s.regular() || !d.regular() || s.total() <= 0) return false;
  const uint32_t g = strided_granule_log(s, d);
  const bool sx = transpose_side(s, d, g), dx = transpose_side(d, s, g);
  if (sx == dx) return false;
  const SideBytes& x = sx ? s : d;
  const SideBytes& y = sx ? d : s;
  if ((s.total() >> g) > kStridedMaxGran) return false;  // k_strided's planner reports the limit
  const int64_t T = tr_tile_side(g);
  out->xbase = x.base;
  out->ybase = y.base;
  out->sb = (uint64_t)x.sb;
  out->R = (uint32_t)x.nb;
  out->C = (uint32_t)x.items;
  out->ntc = fast_div((uint32_t)((x.items + T - 1) / T));
  out->glog = g;
  out->gather = sx ? 1u : 0u;
  return true;
}

// ---- launch tables (as plan_strided_tables) -------------------------------------------------------------------

constexpr int kTransposeMax = 32;  // segments per launch table (the table is a kernel argument: 4 KiB at most)

struct TransposeTable {
  TransposeSeg seg[kTransposeMax];
  uint32_t tile0[kTransposeMax + 1];  // tile0[c] = first block of segment c; tile0[n] = the grid
  int n = 0;
};
static_assert(sizeof(TransposeTable) <= 4096, "the table is a kernel argument");

inline void plan_transpose_tables(const std::vector<TransposeSeg>& segs, std::vector<TransposeTable>* out,
                                  int64_t max_tiles = kMoveMaxTiles) {
  out->clear();
  TransposeTable t;
  t.tile0[0] = 0;
  auto close = [&] {
    if (t.n > 0) out->push_back(t);
    t.n = 0;
    t.tile0[0] = 0;
  };
  for (const TransposeSeg& s : segs) {
    const int64_t tiles = tr_tiles(s);
    if (t.n == kTransposeMax || (int64_t)t.tile0[t.n] + tiles > max_tiles) close();
    t.seg[t.n] = s;
    t.tile0[t.n + 1] = t.tile0[t.n] + (uint32_t)tiles;
    t.n++;
  }
  close();
}

}  // namespace mpjx
