// moves_plan_test.cpp — the host-side planner of the block-move collectives and k_moves' tile geometry
// (mpjexpress_amd/csrc/mpjx_moves_plan.hpp), on the CPU. A stand-alone program: plain g++, no HIP, so it
// also runs under -fsanitize=address,undefined (tests/test_moves_abi.py).
//   - for P in {1, 3, 8, 9, 64}: the tiles of the P x P ragged all-to-all's launch tables cover every
//     segment's bytes exactly once (walked with the functions the kernel itself calls), no tile belongs to
//     an empty segment, no table holds more than kMoveMax segments, and the tables keep the segments' order
//   - every (src mod 16, dst mod 16) pair at the lengths that take another path through a tile
//   - overlapping receive segments, send/receive overlap and negative values are rejected
//   - 2^31 + 5 doubles plan in 64-bit arithmetic (planned only: no memory is allocated)
//   - alltoallv.java's shape at 3 tasks yields the byte ranges its tables imply
#include <stdio.h>
#include <stdlib.h>

#include "../../mpjexpress_amd/csrc/mpjx_moves_plan.hpp"

using namespace mpjx;

static int failures = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
      failures++;                                                       \
    }                                                                   \
  } while (0)

static int64_t ragged(int i, int j) { return (7 * i + 3 * j) % 5 == 0 ? 0 : 1 + ((131 * i + 71 * j) % 97); }

// Walks one launch table as the kernel does: block g -> (segment c, tile x) by the same search, then the
// tile's byte ranges. Returns false unless, per segment, the ranges abut from 0 to its length in tile order
// (every byte exactly once: tiles are visited in increasing g, so a gap or an overlap breaks the chain).
static bool walk_table(const MoveTable& t, int64_t vecs) {
  if (t.n < 1 || t.n > kMoveMax || t.tile0[0] != 0) return false;
  std::vector<int64_t> covered((size_t)t.n, 0);
  for (uint32_t g = 0; g < t.tile0[t.n]; g++) {
    int c = 0, hi = t.n;
    while (hi - c > 1) {
      const int mid = (c + hi) >> 1;
      if (t.tile0[mid] <= g) c = mid;
      else hi = mid;
    }
    if (!(t.tile0[c] <= g && g < t.tile0[c + 1])) return false;
    const MoveSeg& sg = t.seg[c];
    if (sg.bytes <= 0) return false;  // a tile of an empty segment
    const int64_t x = g - t.tile0[c], last = (int64_t)(t.tile0[c + 1] - t.tile0[c]) - 1;
    const MoveGeom gm = move_geom(sg.dst, sg.bytes);
    int64_t v0, v1;
    move_tile_vectors(gm, x, vecs, &v0, &v1);
    int64_t& at = covered[(size_t)c];
    if (x == 0) {  // head [0, head)
      if (at != 0) return false;
      at = gm.head;
    }
    if (v0 < v1) {  // whole vectors: 16 B each, aligned in the destination, inside the segment
      const int64_t lo = 16 * v0 - gm.da, end = 16 * v1 - gm.da;
      if (lo != at || lo < 0 || end > sg.bytes || ((sg.dst + (uint64_t)lo) & 15u) != 0) return false;
      at = end;
    }
    if (x == last) {  // tail [ts, n)
      if (gm.ts != at || sg.bytes - gm.ts >= 16 || gm.ts > sg.bytes) return false;
      at = sg.bytes;
    }
  }
  for (int c = 0; c < t.n; c++) {
    if (t.tile0[c + 1] <= t.tile0[c]) return false;  // a segment without a tile
    if (covered[(size_t)c] != t.seg[c].bytes) return false;
  }
  return true;
}

static void check_plan(const std::vector<MoveSeg>& segs, int64_t vecs, int64_t max_tiles = kMoveMaxTiles) {
  std::vector<MoveTable> tabs;
  plan_tables(segs, vecs, &tabs, max_tiles);
  // the tables, read back in order, are the non-empty segments in order (cut only at tile boundaries)
  size_t k = 0;
  int64_t done = 0;
  bool order = true;
  for (const MoveTable& t : tabs) {
    EXPECT(walk_table(t, vecs));
    EXPECT((int64_t)t.tile0[t.n] <= max_tiles);
    for (int c = 0; c < t.n; c++) {
      while (k < segs.size() && segs[k].bytes <= 0) k++;
      if (k == segs.size()) { order = false; break; }
      const MoveSeg& s = segs[k];
      order = order && t.seg[c].src == s.src + (uint64_t)done && t.seg[c].dst == s.dst + (uint64_t)done;
      done += t.seg[c].bytes;
      if (done == s.bytes) { k++; done = 0; }
      else if (done > s.bytes) order = false;
    }
  }
  while (k < segs.size() && segs[k].bytes <= 0) k++;
  EXPECT(order && k == segs.size() && done == 0);
}

static void world_tables() {
  const int esz = 4;
  for (int P : {1, 3, 8, 9, 64}) {
    // every rank's alltoallv tables, stride 113 elements, buffers at odd addresses
    std::vector<std::vector<ByteRange>> S((size_t)P), R((size_t)P);
    std::string err;
    for (int r = 0; r < P; r++) {
      std::vector<int64_t> sc((size_t)P), sd((size_t)P), rc((size_t)P), rd((size_t)P);
      for (int j = 0; j < P; j++) {
        sc[(size_t)j] = ragged(r, j);
        rc[(size_t)j] = ragged(j, r);
        sd[(size_t)j] = 113 * (int64_t)(P - 1 - j) + 1;
        rd[(size_t)j] = 113 * (int64_t)(P - 1 - j) + 2;
      }
      EXPECT(plan_ranges(sc.data(), sd.data(), P, esz, &S[(size_t)r], &err));
      EXPECT(plan_ranges(rc.data(), rd.data(), P, esz, &R[(size_t)r], &err));
      int a, b;
      EXPECT(!ranges_overlap(R[(size_t)r], &a, &b));
    }
    std::vector<MoveSeg> segs;
    int64_t nonempty = 0;
    for (int j = 0; j < P; j++)
      for (int i = 0; i < P; i++) {
        EXPECT(S[(size_t)i][(size_t)j].len == R[(size_t)j][(size_t)i].len);
        const uint64_t src = 0x7f0000000003ull + (uint64_t)i * 0x100000 + (uint64_t)S[(size_t)i][(size_t)j].off;
        const uint64_t dst = 0x7e0000000005ull + (uint64_t)j * 0x100000 + (uint64_t)R[(size_t)j][(size_t)i].off;
        segs.push_back(MoveSeg{src, dst, R[(size_t)j][(size_t)i].len});
        nonempty += R[(size_t)j][(size_t)i].len > 0;
      }
    for (int64_t vecs : {(int64_t)512, (int64_t)1024, (int64_t)2}) {
      std::vector<MoveTable> tabs;
      plan_tables(segs, vecs, &tabs);
      int64_t held = 0;
      for (const MoveTable& t : tabs) held += t.n;
      EXPECT(held == nonempty);
      EXPECT((int64_t)tabs.size() == (nonempty + kMoveMax - 1) / kMoveMax);
      check_plan(segs, vecs);
    }
    // the equal-count all-to-all: P x P segments of 1031 ints, ceil(P^2 / kMoveMax) tables (2 at P = 9)
    std::vector<ByteRange> E;
    EXPECT(plan_equal(1031, P, esz, &E, &err));
    segs.clear();
    for (int j = 0; j < P; j++)
      for (int i = 0; i < P; i++)
        segs.push_back(MoveSeg{0x7f0000000000ull + (uint64_t)i * 0x100000 + (uint64_t)E[(size_t)j].off,
                               0x7e0000000004ull + (uint64_t)j * 0x100000 + (uint64_t)E[(size_t)i].off,
                               E[(size_t)i].len});
    std::vector<MoveTable> tabs;
    plan_tables(segs, 1024, &tabs);
    EXPECT((int64_t)tabs.size() == ((int64_t)P * P + kMoveMax - 1) / kMoveMax);
    check_plan(segs, 1024);
  }
}

static void alignment_pairs() {
  std::vector<MoveSeg> segs;
  for (uint64_t a = 0; a < 16; a++)
    for (uint64_t b = 0; b < 16; b++)
      for (int64_t n : {0, 1, 15, 16, 17, 31, 33, 4099, 70001})
        segs.push_back(MoveSeg{0x10000 + a, 0x900000 + b, n});
  check_plan(segs, 1024);
  check_plan(segs, 512);
  check_plan(segs, 3);
  check_plan(segs, 3, 7);  // long segments cut into pieces of at most 7 tiles
  // the geometry's corner values
  MoveGeom g = move_geom(5, 3);  // inside one vector: all head
  EXPECT(g.head == 3 && g.ve <= g.vb && g.ts == 3 && g.nvec == 1);
  g = move_geom(0, 5);  // aligned, shorter than a vector: all tail
  EXPECT(g.head == 0 && g.ve == 0 && g.ts == 0);
  g = move_geom(5, 20);  // head 11, no whole vector, tail 9
  EXPECT(g.head == 11 && g.ve == 1 && g.vb == 1 && g.ts == 11 && g.nvec == 2);
  g = move_geom(16, 32);
  EXPECT(g.head == 0 && g.vb == 0 && g.ve == 2 && g.ts == 32 && g.nvec == 2);
  EXPECT(move_tiles(0, 0, 512) == 0 && move_tiles(7, 1, 512) == 1 && move_tiles(0, 8192, 512) == 1 &&
         move_tiles(1, 8192, 512) == 2);
}

static void rejections() {
  std::vector<ByteRange> r;
  std::string err;
  const int64_t c1[3] = {4, -1, 4}, d1[3] = {0, 8, 16};
  EXPECT(!plan_ranges(c1, d1, 3, 4, &r, &err) && err.find("negative") != std::string::npos);
  const int64_t c2[3] = {4, 4, 4}, d2[3] = {0, -8, 16};
  EXPECT(!plan_ranges(c2, d2, 3, 4, &r, &err) && err.find("displacement") != std::string::npos);
  const int64_t c3[2] = {INT64_MAX / 2, 1}, d3[2] = {0, 0};
  EXPECT(!plan_ranges(c3, d3, 2, 16, &r, &err));
  EXPECT(!plan_equal(-3, 4, 8, &r, &err));
  EXPECT(!plan_equal(INT64_MAX / 8, 64, 8, &r, &err));
  // overlapping receive segments: [0, 16) and [8, 24) bytes; an empty one inside another is no overlap
  const int64_t c4[3] = {4, 4, 0}, d4[3] = {0, 2, 1};
  EXPECT(plan_ranges(c4, d4, 3, 4, &r, &err));
  int a = -1, b = -1;
  EXPECT(ranges_overlap(r, &a, &b) && a == 0 && b == 1);
  const int64_t d5[3] = {4, 0, 1};  // abutting, in descending order
  EXPECT(plan_ranges(c4, d5, 3, 4, &r, &err) && !ranges_overlap(r, &a, &b));
  // send against receive
  std::vector<ByteRange> s{{0, 16}}, q{{0, 16}};
  EXPECT(ranges_cross(1000, s, 1015, q) && !ranges_cross(1000, s, 1016, q) && !ranges_cross(1016, s, 1000, q));
  std::vector<ByteRange> e{{0, 0}};
  EXPECT(!ranges_cross(1000, e, 1000, q));
}

static void beyond_32_bits() {
  const int64_t count = ((int64_t)1 << 31) + 5;  // doubles: 16 GiB + 40 B
  std::vector<ByteRange> r;
  std::string err;
  const int64_t d = 3;
  EXPECT(plan_ranges(&count, &d, 1, 8, &r, &err));
  EXPECT(r[0].off == 24 && r[0].len == count * 8 && r[0].len > ((int64_t)1 << 34));
  EXPECT(plan_equal(count, 3, 8, &r, &err) && r[2].off == 2 * count * 8);
  std::vector<MoveSeg> segs{MoveSeg{0x7f0000000000ull + 1, 0x700000000000ull + 24, count * 8}};
  std::vector<MoveTable> tabs;
  plan_tables(segs, 512, &tabs);
  EXPECT(tabs.size() == 1 && tabs[0].n == 1);
  EXPECT((int64_t)tabs[0].tile0[1] == (8 + count * 8 + 15) / 16 / 512 + 1);  // 2097153 tiles of 8 KiB
  EXPECT(tabs[0].tile0[1] == 2097153u);
  check_plan(segs, 512);
  check_plan(segs, 512, 1 << 20);  // and cut at a launch's tile limit: three pieces
  plan_tables(segs, 512, &tabs, 1 << 20);
  EXPECT(tabs.size() == 3);
}

// alltoallv.java at 3 tasks: stride 15 ints, rank 0 sends 10 to everyone, everyone's recvcounts[0] = 10
static void reference_shape() {
  const int P = 3, esz = 4;
  for (int me = 0; me < P; me++) {
    int64_t sc[3], sd[3], rc[3], rd[3];
    for (int j = 0; j < P; j++) {
      sc[j] = me == 0 ? 10 : 15;
      sd[j] = j * 15;
      rc[j] = j == 0 ? 10 : 15;
      rd[j] = j * 15;
    }
    std::vector<ByteRange> S, R;
    std::string err;
    EXPECT(plan_ranges(sc, sd, P, esz, &S, &err) && plan_ranges(rc, rd, P, esz, &R, &err));
    for (int j = 0; j < P; j++) {
      EXPECT(S[(size_t)j].off == 60 * j && S[(size_t)j].len == (me == 0 ? 40 : 60));
      EXPECT(R[(size_t)j].off == 60 * j && R[(size_t)j].len == (j == 0 ? 40 : 60));
      // the block from rank j to rank me goes from byte 60 me of j's buffer to byte 60 j of me's:
      // mutually misaligned by 12 (me - j) mod 16 when both buffers are 16-B aligned
      const unsigned mis = (unsigned)((60 * me - 60 * j) & 15);
      EXPECT(mis == (unsigned)((12 * (me - j)) & 15));
    }
    int a, b;
    EXPECT(!ranges_overlap(R, &a, &b));
  }
}

int main() {
  world_tables();
  alignment_pairs();
  rejections();
  beyond_32_bits();
  reference_shape();
  if (failures) {
    printf("moves_plan_test: %d FAILED\n", failures);
    return 1;
  }
  printf("moves_plan_test: ok\n");
  return 0;
}
