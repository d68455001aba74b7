// strided_plan_test.cpp — the derived datatypes' normal form and the host-side planner of the strided block
// moves with k_strided's geometry (mpjexpress_amd/csrc/mpjx_strided_plan.hpp), on the CPU. A stand-alone
// program: plain g++, no HIP, so it also runs under -fsanitize=address,undefined (tests/test_strided_abi.py).
//   - the normal form: Vector(c, b, b), count <= 1, pair and contiguous derived oldtypes, the rejections
//   - the reciprocal division against `/` at the edges of its range
//   - for P in {1, 3, 9, 64} with ragged counts: walked with the functions the kernel calls, every packed
//     granule of every segment belongs to exactly one (tile, lane, step) and maps to the source and
//     destination addresses that plain indexing gives; no tile belongs to an empty segment; tables split at
//     kStridedMax segments and at the tile limit
//   - granule selection reaches each of 1, 2, 4, 8 and 16 B
//   - 2^31 + 5 blocks plan in 64-bit arithmetic (planned only: no memory is allocated)
//   - the exact overlap check accepts interleaved columns, rejects one column twice and a send layout over
//     a receive layout; beyond kOverlapMaxBlocks blocks it is switched off and does not reject
#include <stdio.h>
#include <stdlib.h>

#include "../../mpjexpress_amd/csrc/mpjx_strided_plan.hpp"

using namespace mpjx;

static int failures = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
      failures++;                                                       \
    }                                                                   \
  } while (0)

static int64_t ragged(int i, int j) { return (7 * i + 3 * j) % 5 == 0 ? 0 : 1 + ((131 * i + 71 * j) % 23); }

static TypeForm basic(int code) {
  TypeForm f;
  EXPECT(basic_form(code, &f));
  return f;
}

static TypeForm vec(int64_t c, int64_t b, int64_t s, const TypeForm& old, int want = kTypeOk) {
  TypeForm f;
  std::string err;
  const int rc = vector_form(c, b, s, old, &f, &err);
  EXPECT(rc == want);
  if (rc != kTypeOk) EXPECT(!err.empty());
  return f;
}

static void test_forms() {
  const TypeForm D = basic(8), I = basic(5), D2 = basic(0x108);
  EXPECT(D.size() == 1 && D.extent() == 1 && D.bsz == 8 && D.contiguous());
  EXPECT(D2.base == 8 && D2.size() == 2 && D2.extent() == 2 && D2.contiguous());
  TypeForm x;
  EXPECT(!basic_form(0, &x) && !basic_form(9, &x) && !basic_form(0x101, &x) && !basic_form(0x104, &x));
  TypeForm v = vec(6, 2, 5, I);
  EXPECT(v.nblocks == 6 && v.blocklen == 2 && v.stride == 5 && v.size() == 12 && v.extent() == 27 && !v.contiguous());
  v = vec(4, 3, 3, I);  // stride == blocklength
  EXPECT(v.contiguous() && v.size() == 12 && v.extent() == 12);
  v = vec(1, 3, -7, I);  // one block: the stride does not matter
  EXPECT(v.contiguous() && v.size() == 3 && v.extent() == 3);
  v = vec(0, 3, 7, I);
  EXPECT(v.size() == 0 && v.extent() == 0 && v.contiguous());
  v = vec(5, 0, 7, I);
  EXPECT(v.size() == 0 && v.extent() == 0);
  v = vec(3, 2, 4, D2);  // stride in pairs
  EXPECT(v.base == 8 && v.nblocks == 3 && v.blocklen == 4 && v.stride == 8 && v.extent() == 20);
  TypeForm c4;
  std::string err;
  EXPECT(contiguous_of(4, I, &c4, &err) == kTypeOk && c4.contiguous() && c4.size() == 4);
  v = vec(3, 2, 5, c4);  // a contiguous derived oldtype
  EXPECT(v.nblocks == 3 && v.blocklen == 8 && v.stride == 20 && v.extent() == 48);
  EXPECT(contiguous_of(0, I, &c4, &err) == kTypeOk && c4.size() == 0);
  EXPECT(contiguous_of(-1, I, &c4, &err) == kTypeErrArg);
  vec(-1, 2, 5, I, kTypeErrArg);
  vec(2, -1, 5, I, kTypeErrArg);
  vec(2, 3, 2, I, kTypeErrUnsupported);   // overlapping
  vec(2, 3, 0, I, kTypeErrUnsupported);   // zero
  vec(2, 3, -4, I, kTypeErrUnsupported);  // negative
  const TypeForm strided = vec(6, 2, 5, I);
  vec(2, 1, 2, strided, kTypeErrUnsupported);  // Vector of Vector
  EXPECT(contiguous_of(2, strided, &c4, &err) == kTypeErrUnsupported);  // Contiguous of Vector
  vec(2, (int64_t)1 << 61, (int64_t)1 << 62, D, kTypeErrArg);  // beyond 2^62 bytes
}

static void test_fastdiv() {
  const uint32_t ds[] = {1, 2, 3, 5, 7, 10, 255, 256, 641, 65535, 65536, 65537, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
  uint64_t r = 88172645463325252ull;
  for (uint32_t d : ds) {
    const FastDiv f = fast_div(d);
    const uint32_t edge[] = {0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    for (uint32_t n : edge) EXPECT(fd_div(f, n) == n / d);
    for (uint64_t k = 1; k * d <= 0xffffffffull && k < 40; k++) {  // around the multiples
      EXPECT(fd_div(f, (uint32_t)(k * d)) == k);
      EXPECT(fd_div(f, (uint32_t)(k * d - 1)) == (k * d - 1) / d);
    }
    const uint64_t top = 0xffffffffull / d * d;  // the largest multiple
    EXPECT(fd_div(f, (uint32_t)top) == top / d);
    if (top > 0) EXPECT(fd_div(f, (uint32_t)(top - 1)) == (top - 1) / d);
    for (int k = 0; k < 2000; k++) {
      r ^= r << 13, r ^= r >> 7, r ^= r << 17;
      const uint32_t n = (uint32_t)r;
      if (fd_div(f, n) != n / d) {
        EXPECT(fd_div(f, n) == n / d);
        break;
      }
    }
  }
}

// Walks one launch table as the kernel does: block g -> (segment c, tile x) by the same search, then every
// lane and step of the tile. Each granule must be reached exactly once, naturally aligned, at the addresses
// the layouts' own indexing (SideBytes::at) gives for its first and last byte.
struct Ref {
  SideBytes s, d;
};

static bool walk_table(const StridedTable& t, const Ref* ref, int64_t lanes, int64_t steps) {
  if (t.n < 1 || t.n > kStridedMax || t.tile0[0] != 0) return false;
  std::vector<std::vector<unsigned char>> hit((size_t)t.n);
  for (int c = 0; c < t.n; c++) {
    if (t.seg[c].ngran == 0 || t.tile0[c + 1] <= t.tile0[c]) return false;  // an empty segment or one without tiles
    if ((int64_t)(t.tile0[c + 1] - t.tile0[c]) != strided_tiles(t.seg[c].ngran, lanes * steps)) return false;
    hit[(size_t)c].assign(t.seg[c].ngran, 0);
  }
  for (uint32_t g = 0; g < t.tile0[t.n]; g++) {
    int c = 0, hi = t.n;
    while (hi - c > 1) {
      const int mid = (c + hi) >> 1;
      if (t.tile0[mid] <= g) c = mid;
      else hi = mid;
    }
    if (!(t.tile0[c] <= g && g < t.tile0[c + 1])) return false;
    const StridedSeg& sg = t.seg[c];
    const uint32_t x = g - t.tile0[c];
    const int64_t G = (int64_t)1 << sg.glog;
    bool any = false;
    for (int64_t u = 0; u < steps; u++)
      for (int64_t lane = 0; lane < lanes; lane++) {
        const uint64_t q = (uint64_t)x * (uint64_t)(lanes * steps) + (uint64_t)(u * lanes + lane);
        if (q >= sg.ngran) continue;
        any = true;
        if (hit[(size_t)c][q]++) return false;
        const uint64_t sa = strided_addr(sg.s, (uint32_t)q, sg.glog), da = strided_addr(sg.d, (uint32_t)q, sg.glog);
        const int64_t p = (int64_t)q * G;
        if (sa != ref[c].s.at(p) || sa + (uint64_t)G - 1 != ref[c].s.at(p + G - 1)) return false;
        if (da != ref[c].d.at(p) || da + (uint64_t)G - 1 != ref[c].d.at(p + G - 1)) return false;
        if ((sa & (uint64_t)(G - 1)) || (da & (uint64_t)(G - 1))) return false;
      }
    if (!any) return false;  // a tile that moves nothing
  }
  for (int c = 0; c < t.n; c++)
    for (unsigned char h : hit[(size_t)c])
      if (h != 1) return false;
  return true;
}

// The P x P ragged all-to-all with a Vector on both sides, of different blocking: rank i sends ragged(i, j)
// items of `st` to rank j, which receives the same number of items of `rt` (equal sizes).
static void test_world(int P, const TypeForm& st, const TypeForm& rt, int64_t soff, int64_t roff, uint32_t want_glog,
                       int64_t gran, int64_t lanes, int64_t max_tiles) {
  std::vector<StridedSeg> segs;
  std::vector<Ref> refs;
  int64_t total = 0;
  int nonempty = 0;
  for (int j = 0; j < P; j++)
    for (int i = 0; i < P; i++) {
      const int64_t n = ragged(i, j);
      SideBytes s, d;
      std::string err;
      const uint64_t sbuf = 0x100000000ull + (uint64_t)i * 0x4000000ull, rbuf = 0x900000000ull + (uint64_t)j * 0x4000000ull;
      EXPECT(plan_side(st, sbuf, n, soff + (int64_t)j * 40 * st.extent(), &s, &err));
      EXPECT(plan_side(rt, rbuf, n, roff + (int64_t)i * 40 * rt.extent(), &d, &err));
      EXPECT(s.total() == d.total() && s.total() == n * st.size() * st.bsz);
      if (n == 0) {
        EXPECT(s.total() == 0 && s.blocks() == 0);
        continue;
      }
      StridedSeg sg;
      EXPECT(plan_strided_seg(s, d, &sg, &err) == kTypeOk);
      EXPECT(sg.glog == want_glog && ((int64_t)sg.ngran << sg.glog) == s.total());
      segs.push_back(sg);
      refs.push_back(Ref{s, d});
      total += s.total();
      nonempty++;
    }
  std::vector<StridedTable> tabs;
  plan_strided_tables(segs, gran, &tabs, max_tiles);
  size_t at = 0;
  int64_t seen = 0;
  for (const StridedTable& t : tabs) {
    EXPECT(t.n >= 1 && t.n <= kStridedMax && (int64_t)t.tile0[t.n] <= std::max<int64_t>(max_tiles, 1));
    EXPECT(at + (size_t)t.n <= refs.size());
    EXPECT(walk_table(t, refs.data() + at, lanes, gran / lanes));
    for (int c = 0; c < t.n; c++) seen += (int64_t)t.seg[c].ngran << t.seg[c].glog;
    at += (size_t)t.n;
  }
  EXPECT(at == (size_t)nonempty && seen == total);
  if (nonempty > kStridedMax && max_tiles == kMoveMaxTiles)
    EXPECT(tabs.size() == (size_t)(nonempty + kStridedMax - 1) / kStridedMax);
}

static SideBytes side(uint64_t base, int64_t bb, int64_t sb, int64_t nb, int64_t items) {
  SideBytes x;
  x.base = base, x.bb = bb, x.sb = sb, x.nb = nb, x.items = items;
  x.eb = (nb - 1) * sb + bb;
  return x;
}

static void test_granules() {
  const SideBytes d = side(0x2000, 960, 960, 1, 1);  // contiguous, 16-B aligned
  EXPECT(strided_granule_log(side(0x1000, 48, 80, 4, 5), d) == 4);
  EXPECT(strided_granule_log(side(0x1008, 48, 80, 4, 5), d) == 3);   // the base
  EXPECT(strided_granule_log(side(0x1000, 24, 80, 4, 10), d) == 3);  // the block
  EXPECT(strided_granule_log(side(0x1000, 48, 84, 4, 5), d) == 2);   // the stride
  EXPECT(strided_granule_log(side(0x1000, 6, 10, 4, 40), d) == 1);
  EXPECT(strided_granule_log(side(0x1000, 3, 7, 5, 64), d) == 0);
  EXPECT(strided_granule_log(side(0x1000, 48, 80, 4, 5), side(0x2001, 960, 960, 1, 1)) == 0);  // the other side
  SideBytes e = side(0x1000, 16, 32, 2, 3);
  e.eb = 52;  // the extent alone
  EXPECT(strided_granule_log(e, side(0x2000, 96, 96, 1, 1)) == 2);
}

static void test_huge() {
  // 2^31 + 5 blocks of one double, every other double: one item of Vector(2^31 + 5, 1, 2, DOUBLE)
  const int64_t nb = ((int64_t)1 << 31) + 5;
  const TypeForm v = vec(nb, 1, 2, basic(8));
  SideBytes s, d;
  std::string err;
  EXPECT(plan_side(v, 0x1000000000ull, 1, 3, &s, &err));
  EXPECT(plan_side(contiguous_form(8, 8, 1), 0x9000000000ull, nb, 1, &d, &err));
  EXPECT(s.total() == nb * 8 && d.total() == nb * 8 && d.contiguous() && s.blocks() == nb);
  StridedSeg sg;
  EXPECT(plan_strided_seg(s, d, &sg, &err) == kTypeOk);
  EXPECT(sg.glog == 3 && (int64_t)sg.ngran == nb);
  EXPECT(strided_tiles(sg.ngran, kStridedTile) == (nb + kStridedTile - 1) / kStridedTile);
  const int64_t qs[] = {0, 1, 1023, 1024, ((int64_t)1 << 31) - 1, (int64_t)1 << 31, nb - 1};
  for (int64_t q : qs) {
    EXPECT(strided_addr(sg.s, (uint32_t)q, 3) == 0x1000000000ull + 24 + (uint64_t)q * 16);
    EXPECT(strided_addr(sg.s, (uint32_t)q, 3) == s.at(q * 8));
    EXPECT(strided_addr(sg.d, (uint32_t)q, 3) == 0x9000000000ull + 8 + (uint64_t)q * 8);
  }
  std::vector<StridedTable> tabs;
  plan_strided_tables(std::vector<StridedSeg>{sg}, kStridedTile, &tabs);
  EXPECT(tabs.size() == 1 && tabs[0].n == 1 && (int64_t)tabs[0].tile0[1] == (nb + kStridedTile - 1) / kStridedTile);
  // disjoint bounding spans settle the overlap question without expanding a block, at any size; with more
  // blocks than the exact check expands and spans that meet, it is switched off, not a rejection
  int a = -1, b = -1;
  EXPECT(strided_overlap(std::vector<SideBytes>{s}, std::vector<SideBytes>{d}, &a, &b) == kNoOverlap);
  SideBytes d2;
  EXPECT(plan_side(contiguous_form(8, 8, 1), 0x1000000000ull, 1, 4, &d2, &err));  // inside a gap of s
  EXPECT(strided_overlap(std::vector<SideBytes>{s}, std::vector<SideBytes>{d2}, &a, &b) == kOverlapUnchecked);
  // 2^32 granules: refused by name, not truncated
  SideBytes bs, bd;
  EXPECT(plan_side(vec((int64_t)1 << 32, 1, 2, basic(1)), 0x1000000001ull, 1, 0, &bs, &err));
  EXPECT(plan_side(contiguous_form(1, 1, 1), 0x9000000000ull, (int64_t)1 << 32, 0, &bd, &err));
  err.clear();
  EXPECT(plan_strided_seg(bs, bd, &sg, &err) == kTypeErrUnsupported && !err.empty());
  // negative values and sizes beyond 2^62
  EXPECT(!plan_side(v, 0, -1, 0, &s, &err) && !plan_side(v, 0, 1, -1, &s, &err));
  EXPECT(!plan_side(v, 0, (int64_t)1 << 40, 0, &s, &err));
}

static void test_overlap() {
  // an 8 x 4 matrix of doubles: column c is Vector(8, 1, 4) at displacement c
  const TypeForm col = vec(8, 1, 4, basic(8));
  const uint64_t rbuf = 0x700000000ull, sbuf = 0x100000000ull;
  auto column = [&](uint64_t buf, int c) {
    SideBytes x;
    std::string err;
    EXPECT(plan_side(col, buf, 1, c, &x, &err));
    return x;
  };
  std::vector<SideBytes> S{column(sbuf, 0), column(sbuf, 1), SideBytes{}};
  int a = -1, b = -1;
  EXPECT(strided_overlap(S, std::vector<SideBytes>{column(rbuf, 0), column(rbuf, 1), column(rbuf, 3)}, &a, &b) == kNoOverlap);
  EXPECT(strided_overlap(S, std::vector<SideBytes>{column(rbuf, 2), column(rbuf, 0), column(rbuf, 2)}, &a, &b) == kRecvOverlap);
  EXPECT((a == 0 && b == 2) || (a == 2 && b == 0));
  // a send column over a receive column of the same matrix; its neighbour column is fine
  EXPECT(strided_overlap(std::vector<SideBytes>{column(rbuf, 1)}, std::vector<SideBytes>{column(rbuf, 0), column(rbuf, 1)}, &a, &b) ==
         kSendRecvOverlap);
  EXPECT(a == 0 && b == 1);
  EXPECT(strided_overlap(std::vector<SideBytes>{column(rbuf, 2)}, std::vector<SideBytes>{column(rbuf, 0), column(rbuf, 1)}, &a, &b) ==
         kNoOverlap);
  // two items of a type: item 1 starts one extent after item 0; a contiguous run inside the gap is fine
  const TypeForm two = vec(2, 2, 6, basic(5));  // extent 8 ints: [0,2) [6,8) | [8,10) [14,16)
  SideBytes x, y;
  std::string err;
  EXPECT(plan_side(two, rbuf, 2, 0, &x, &err) && plan_side(contiguous_form(5, 4, 1), rbuf, 4, 2, &y, &err));
  EXPECT(strided_overlap({}, std::vector<SideBytes>{x, y}, &a, &b) == kNoOverlap);
  EXPECT(plan_side(contiguous_form(5, 4, 1), rbuf, 5, 2, &y, &err));  // one int further: into [6, 8)
  EXPECT(strided_overlap({}, std::vector<SideBytes>{x, y}, &a, &b) == kRecvOverlap);
  // the cap: 65,536 blocks are still checked, one more is not
  const TypeForm big = vec(kOverlapMaxBlocks / 2, 1, 2, basic(1));
  EXPECT(plan_side(big, rbuf, 1, 0, &x, &err));
  EXPECT(strided_overlap({}, std::vector<SideBytes>{x, x}, &a, &b) == kRecvOverlap);
  EXPECT(plan_side(vec(kOverlapMaxBlocks / 2 + 1, 1, 2, basic(1)), rbuf, 1, 0, &y, &err));
  EXPECT(strided_overlap({}, std::vector<SideBytes>{x, y}, &a, &b) == kOverlapUnchecked);
}

int main() {
  test_forms();
  test_fastdiv();
  const TypeForm I = basic(5), B = basic(1), C = basic(2), D = basic(8), D2 = basic(0x108);
  for (int P : {1, 3, 9, 64}) {
    // INT, different blocking on the two sides, odd offsets: granule 4
    test_world(P, vec(6, 2, 5, I), vec(4, 3, 7, I), 1, 3, 2, kStridedTile, 256, kMoveMaxTiles);
    // BYTE at odd offsets: granule 1; the streaming form's tile
    test_world(P, vec(5, 3, 7, B), contiguous_form(1, 1, 15), 3, 1, 0, kStridedTileNT, 512, kMoveMaxTiles);
    // CHAR: granule 2
    test_world(P, vec(4, 3, 5, C), vec(2, 6, 9, C), 1, 0, 1, kStridedTile, 256, kMoveMaxTiles);
    // DOUBLE columns into contiguous rows: granule 8
    test_world(P, vec(33, 1, 17, D), contiguous_form(8, 8, 33), 1, 0, 3, kStridedTile, 256, kMoveMaxTiles);
    // DOUBLE2 pairs at even offsets: granule 16
    test_world(P, vec(3, 2, 4, D2), vec(2, 3, 5, D2), 2, 4, 4, kStridedTile, 256, kMoveMaxTiles);
  }
  // tables also close at the tile limit: long segments, two tiles per table at most
  test_world(9, vec(300, 2, 5, I), vec(200, 3, 7, I), 0, 0, 2, kStridedTile, 256, 40);
  test_granules();
  test_huge();
  test_overlap();
  if (failures) {
    printf("strided_plan_test: %d failures\n", failures);
    return 1;
  }
  printf("strided_plan_test: ok\n");
  return 0;
}
