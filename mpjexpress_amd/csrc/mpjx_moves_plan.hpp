// mpjx_moves_plan.hpp — host-side planning of the block-move collectives (Allgather(v), Gatherv,
// Scatterv, Alltoall(v)) and the tile geometry of k_moves (mpjx_k_moves.hip). No HIP include: plain
// C++17, so the planner is compiled, tested and sanitized on the CPU (tests/cpp/moves_plan_test.cpp);
// the kernel includes the same header, so the geometry the test walks is the geometry the kernel runs.
//
// A move is one segment (src, dst, bytes) with any alignment pair. The kernel works in the
// DESTINATION's 16-B vector grid: vector v of a segment is the aligned 16 B at (dst & ~15) + 16 v.
//   head  the bytes before the first whole vector (dst up to its 16-B alignment), at most 15
//   body  the whole vectors: one aligned 16-B store each
//   tail  the bytes after the last whole vector, at most 15
// A tile is `vecs` consecutive vectors; the first tile also moves the head, the last the tail. The
// launch table holds up to kMoveMax segments and the prefix sum of their tile counts, so block g of a
// launch finds its (segment, tile) by a search over at most kMoveMax + 1 numbers, and no block exists
// for a tile that does not. All byte arithmetic is 64-bit.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MPJX_HD __host__ __device__
#else
#define MPJX_HD
#endif

namespace mpjx {

// ---- tile geometry (shared with the kernel) -------------------------------------------------------

struct MoveGeom {
  unsigned da;   // dst & 15
  int64_t head;  // bytes [0, head) are moved byte-wise by tile 0
  int64_t vb, ve;  // whole vectors [vb, ve): vector v holds segment bytes [16 v - da, 16 v - da + 16)
  int64_t ts;    // bytes [ts, n) are moved byte-wise by the last tile (n - ts < 16)
  int64_t nvec;  // vectors touched, whole or not: the tile count is ceil(nvec / vecs)
};

MPJX_HD inline MoveGeom move_geom(uint64_t dst, int64_t n) {
  MoveGeom g;
  g.da = (unsigned)(dst & 15u);
  const int64_t to_al = (int64_t)((16u - g.da) & 15u);
  g.head = n < to_al ? n : to_al;
  g.vb = g.da ? 1 : 0;
  g.ve = ((int64_t)g.da + n) >> 4;
  const int64_t body_end = g.ve > g.vb ? 16 * g.ve - (int64_t)g.da : g.head;
  g.ts = body_end > g.head ? body_end : g.head;
  g.nvec = ((int64_t)g.da + n + 15) >> 4;
  return g;
}

// Tiles of a segment of n bytes stored at address dst, `vecs` vectors per tile; 0 for an empty segment.
MPJX_HD inline int64_t move_tiles(uint64_t dst, int64_t n, int64_t vecs) {
  if (n <= 0) return 0;
  const int64_t nvec = ((int64_t)(dst & 15u) + n + 15) >> 4;
  return (nvec + vecs - 1) / vecs;
}

// The whole vectors [*v0, *v1) of tile x (empty when *v0 >= *v1)
MPJX_HD inline void move_tile_vectors(const MoveGeom& g, int64_t x, int64_t vecs, int64_t* v0, int64_t* v1) {
  const int64_t a = x * vecs, b = a + vecs;
  *v0 = a > g.vb ? a : g.vb;
  *v1 = b < g.ve ? b : g.ve;
}

// ---- counts and displacements -> byte ranges ----------------------------------------------------------

struct ByteRange {
  int64_t off, len;  // bytes from the buffer's base
};

constexpr int64_t kMoveMaxBytes = (int64_t)1 << 62;

// ranges[j] = (displs[j] * esz, counts[j] * esz) for j < n (displs == nullptr: every displacement 0).
// False with *err set for a negative value or a product beyond 2^62.
inline bool plan_ranges(const int64_t* counts, const int64_t* displs, int n, int esz, std::vector<ByteRange>* out,
                        std::string* err, const char* what = "count") {
  out->assign((size_t)n, ByteRange{0, 0});
  if (esz <= 0) {
    *err = "element size must be positive";
    return false;
  }
  for (int j = 0; j < n; j++) {
    const int64_t c = counts[j], d = displs ? displs[j] : 0;
    if (c < 0 || d < 0) {
      *err = std::string("negative ") + (c < 0 ? what : "displacement") + " at index " + std::to_string(j);
      return false;
    }
    if (c > kMoveMaxBytes / esz || d > kMoveMaxBytes / esz) {
      *err = std::string(what) + " or displacement too large at index " + std::to_string(j);
      return false;
    }
    (*out)[(size_t)j] = ByteRange{d * esz, c * esz};
  }
  return true;
}

// Equal blocks of `count` elements, block j at j * count.
inline bool plan_equal(int64_t count, int n, int esz, std::vector<ByteRange>* out, std::string* err) {
  std::vector<int64_t> c((size_t)n, count), d((size_t)n);
  if (count < 0) {
    *err = "negative count";
    return false;
  }
  if (n > 0 && count > kMoveMaxBytes / esz / n) {
    *err = "count too large";
    return false;
  }
  for (int j = 0; j < n; j++) d[(size_t)j] = (int64_t)j * count;
  return plan_ranges(c.data(), d.data(), n, esz, out, err);
}

// True (and *a, *b = the indices) if two non-empty ranges of the list share a byte.
inline bool ranges_overlap(const std::vector<ByteRange>& r, int* a, int* b) {
  std::vector<int> idx;
  for (int j = 0; j < (int)r.size(); j++)
    if (r[(size_t)j].len > 0) idx.push_back(j);
  std::sort(idx.begin(), idx.end(), [&](int x, int y) { return r[(size_t)x].off < r[(size_t)y].off; });
  for (size_t k = 1; k < idx.size(); k++) {
    const ByteRange& p = r[(size_t)idx[k - 1]];
    if (p.off + p.len > r[(size_t)idx[k]].off) {
      *a = idx[k - 1];
      *b = idx[k];
      return true;
    }
  }
  return false;
}

// True if a non-empty range of `s` at base address sbase shares a byte with one of `r` at rbase.
inline bool ranges_cross(uint64_t sbase, const std::vector<ByteRange>& s, uint64_t rbase,
                         const std::vector<ByteRange>& r) {
  for (const ByteRange& x : s) {
    if (x.len <= 0) continue;
    const uint64_t x0 = sbase + (uint64_t)x.off, x1 = x0 + (uint64_t)x.len;
    for (const ByteRange& y : r) {
      if (y.len <= 0) continue;
      const uint64_t y0 = rbase + (uint64_t)y.off, y1 = y0 + (uint64_t)y.len;
      if (x0 < y1 && y0 < x1) return true;
    }
  }
  return false;
}

// ---- segments -> launch tables ----------------------------------------------------------------------

struct MoveSeg {
  uint64_t src, dst;  // addresses
  int64_t bytes;
};

constexpr int kMoveMax = 64;                          // segments per launch table
constexpr int64_t kMoveMaxTiles = (int64_t)1 << 30;  // tiles (= blocks) per launch

struct MoveTable {
  MoveSeg seg[kMoveMax];
  uint32_t tile0[kMoveMax + 1];  // tile0[c] = first block of segment c; tile0[n] = the grid
  int n = 0;
};

// The launch tables of `segs` for tiles of `vecs` vectors, in order: empty segments are dropped, a
// segment of more than max_tiles tiles is cut at tile boundaries, and a table is closed when it holds
// kMoveMax segments or max_tiles tiles. Every table has n >= 1 and tile0[n] >= 1.
inline void plan_tables(const std::vector<MoveSeg>& segs, int64_t vecs, std::vector<MoveTable>* out,
                        int64_t max_tiles = kMoveMaxTiles) {
  out->clear();
  MoveTable t;
  t.tile0[0] = 0;
  auto close = [&] {
    if (t.n > 0) out->push_back(t);
    t.n = 0;
    t.tile0[0] = 0;
  };
  auto put = [&](uint64_t src, uint64_t dst, int64_t bytes) {
    const int64_t tiles = move_tiles(dst, bytes, vecs);
    if (t.n == kMoveMax || (int64_t)t.tile0[t.n] + tiles > max_tiles) close();
    t.seg[t.n] = MoveSeg{src, dst, bytes};
    t.tile0[t.n + 1] = t.tile0[t.n] + (uint32_t)tiles;
    t.n++;
  };
  for (const MoveSeg& s : segs) {
    if (s.bytes <= 0) continue;
    uint64_t src = s.src, dst = s.dst;
    int64_t left = s.bytes;
    while (move_tiles(dst, left, vecs) > max_tiles) {
      // max_tiles whole tiles from dst: the cut falls on the destination's vector grid
      const int64_t piece = max_tiles * vecs * 16 - (int64_t)(dst & 15u);
      put(src, dst, piece);
      src += (uint64_t)piece;
      dst += (uint64_t)piece;
      left -= piece;
    }
    put(src, dst, left);
  }
  close();
}

}  // namespace mpjx
