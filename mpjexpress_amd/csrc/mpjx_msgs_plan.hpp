// mpjx_msgs_plan.hpp — the launch table and the two address mappings of k_msgs (mpjx_k_msgs.hip): a batch of
// matched point-to-point messages of mixed layout kinds in ONE launch. No HIP include: plain C++17, compiled,
// tested and sanitized on the CPU (tests/cpp/msgs_plan_test.cpp); the kernel includes the same header, so the
// mapping the test walks is the mapping the kernel runs.
//
// A segment is one message and carries a kind, uniform per workgroup:
//   bytes    both layouts contiguous, at any pair of byte alignments: k_moves' destination-grid geometry
//            (move_geom, mpjx_moves_plan.hpp): head and tail byte-wise, one aligned 16-B store per whole vector
//   granule  either side regular (StridedSide) or irregular (IndexedSide, its device table searched directly
//            with indexed_addr: no LDS form); one lane moves one granule, the granule chosen per segment by
//            strided_granule_log
// The grid is the sum of the segments' tiles (tile0[], as k_strided): block g searches the prefix for its
// (segment, tile). A tile is kStridedTile vectors (bytes) or granules (granule); kStridedTileNT in the streaming
// form. A message may be shorter than the receive layout: the segment's length is the sender's packed bytes.
#pragma once
#include "mpjx_indexed_plan.hpp"

namespace mpjx {

constexpr uint32_t kMsgBytes = 0, kMsgGranule = 1;

struct MsgSeg {
  IndexedSeg g;    // granule kind; bytes kind: g.s.r.base = src, g.d.r.base = dst
  int64_t bytes;   // bytes kind: the length
  uint32_t kind;
  uint32_t pad_;
};

constexpr int kMsgsMax = 24;  // segments per launch table (the table is a kernel argument: 4 KiB at most)

struct MsgsTable {
  MsgSeg seg[kMsgsMax];
  uint32_t tile0[kMsgsMax + 1];  // tile0[c] = first block of segment c; tile0[n] = the grid
  int n = 0;
};
static_assert(sizeof(MsgsTable) <= 4096, "the table is a kernel argument");

inline MsgSeg msg_bytes_seg(uint64_t src, uint64_t dst, int64_t bytes) {
  MsgSeg m{};
  m.kind = kMsgBytes;
  m.g.s.r.base = src;
  m.g.d.r.base = dst;
  m.bytes = bytes;
  return m;
}

// The segment of the message s -> d (s.total() > 0 packed bytes; d holds at least as many). stab / dtab are the
// device tables of the irregular sides (plan_indexed_seg).
inline int plan_msg_seg(const SideBytes& s, const IdxEnt* stab, const SideBytes& d, const IdxEnt* dtab, MsgSeg* out,
                        std::string* err) {
  if (s.contiguous() && d.contiguous()) {
    *out = msg_bytes_seg(s.base, d.base, s.total());
    return kTypeOk;
  }
  MsgSeg m{};
  m.kind = kMsgGranule;
  const int rc = plan_indexed_seg(s, stab, d, dtab, &m.g, err);
  if (rc != kTypeOk) return rc;
  m.bytes = (int64_t)m.g.ngran << m.g.glog;
  *out = m;
  return kTypeOk;
}

MPJX_HD inline int64_t msg_tiles(const MsgSeg& m, int64_t tile) {
  return m.kind == kMsgBytes ? move_tiles(m.g.d.r.base, m.bytes, tile) : strided_tiles(m.g.ngran, tile);
}

// The launch tables of `segs` for tiles of `tile` vectors or granules, in order, as plan_tables makes them:
// empty segments are dropped, a bytes segment of more than max_tiles tiles is cut at tile boundaries (a granule
// segment has fewer than 2^32 / tile tiles), and a table is closed when it holds kMsgsMax segments or max_tiles
// tiles. Every table has n >= 1 and tile0[n] >= 1.
inline void plan_msgs_tables(const std::vector<MsgSeg>& segs, int64_t tile, std::vector<MsgsTable>* out,
                             int64_t max_tiles = kMoveMaxTiles) {
  out->clear();
  MsgsTable t;
  t.tile0[0] = 0;
  auto close = [&] {
    if (t.n > 0) out->push_back(t);
    t.n = 0;
    t.tile0[0] = 0;
  };
  auto put = [&](const MsgSeg& m) {
    const int64_t tiles = msg_tiles(m, tile);
    if (t.n == kMsgsMax || (int64_t)t.tile0[t.n] + tiles > max_tiles) close();
    t.seg[t.n] = m;
    t.tile0[t.n + 1] = t.tile0[t.n] + (uint32_t)tiles;
    t.n++;
  };
  for (const MsgSeg& s : segs) {
    if (s.bytes <= 0) continue;
    if (s.kind != kMsgBytes) {
      put(s);
      continue;
    }
    uint64_t src = s.g.s.r.base, dst = s.g.d.r.base;
    int64_t left = s.bytes;
    while (move_tiles(dst, left, tile) > max_tiles) {
      // max_tiles whole tiles from dst: the cut falls on the destination's vector grid
      const int64_t piece = max_tiles * tile * 16 - (int64_t)(dst & 15u);
      put(msg_bytes_seg(src, dst, piece));
      src += (uint64_t)piece;
      dst += (uint64_t)piece;
      left -= piece;
    }
    put(msg_bytes_seg(src, dst, left));
  }
  close();
}

// ---- what one lane does (shared by the kernel and the CPU walk) -------------------------------------------------

// bytes kind, tile x of `last + 1` tiles, lane slot i (0 .. tile): the whole vector it moves, if any. The
// destination vector is the aligned 16 B at (dst & ~15) + 16 v; its source bytes start at src - (dst & 15) + 16 v.
struct MsgVec {
  bool on;
  uint64_t dst, src;  // dst 16-B aligned
};
MPJX_HD inline MsgVec msg_bytes_vec(const MsgSeg& m, const MoveGeom& gm, int64_t x, int64_t tile, int64_t i) {
  int64_t v0, v1;
  move_tile_vectors(gm, x, tile, &v0, &v1);
  const int64_t v = x * tile + i;
  MsgVec r;
  r.on = v >= v0 && v < v1;
  r.dst = m.g.d.r.base - gm.da + (uint64_t)(16 * v);
  r.src = m.g.s.r.base - gm.da + (uint64_t)(16 * v);
  return r;
}

}  // namespace mpjx
