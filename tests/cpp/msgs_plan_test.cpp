// CPU test of k_msgs' launch table and its two address mappings (mpjexpress_amd/csrc/mpjx_msgs_plan.hpp): plain
// C++17, no HIP. Every packed byte of a segment is walked, lane by lane as the kernel does it, against
// SideBytes::at. Built by the Makefile with g++, and by tests/test_p2p_abi.py under the sanitizers.
// With --cases it plans the cases given on stdin instead and prints each one's cell (run_cases below;
// tests/test_msgs_cases.py feeds it tests/msgs_cases.py).
#include <stdio.h>
#include <string.h>

#include <iostream>
#include <map>

#include "../../mpjexpress_amd/csrc/mpjx_msgs_plan.hpp"
#include "../../mpjexpress_amd/csrc/mpjx_transpose_plan.hpp"

using namespace mpjx;

static int g_fail = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      g_fail++;                                                  \
    }                                                            \
  } while (0)

static SideBytes run(uint64_t base, int64_t bytes) {
  SideBytes x;
  x.base = base;
  x.bb = x.sb = x.eb = bytes;
  x.nb = x.items = 1;
  return x;
}

// What the kernel does with one table, as a map destination byte -> source byte; every destination byte at most
// once (CHECKed)
using ByteMap = std::map<uint64_t, uint64_t>;
static void put(ByteMap* m, uint64_t d, uint64_t s) { CHECK(m->emplace(d, s).second); }

static void walk_table(const MsgsTable& t, int64_t tile, ByteMap* out) {
  const int64_t lanes = tile == kStridedTile ? 256 : 512;
  for (uint32_t g = 0; g < t.tile0[t.n]; g++) {
    int c = 0, hi = t.n;
    while (hi - c > 1) {
      const int mid = (c + hi) >> 1;
      if (t.tile0[mid] <= g) c = mid;
      else hi = mid;
    }
    CHECK(t.tile0[c] <= g && g < t.tile0[c + 1]);
    const MsgSeg& m = t.seg[c];
    const int64_t x = g - t.tile0[c], last = (int64_t)(t.tile0[c + 1] - t.tile0[c]) - 1;
    if (m.kind == kMsgBytes) {
      const uint64_t src = m.g.s.r.base, dst = m.g.d.r.base;
      const MoveGeom gm = move_geom(dst, m.bytes);
      for (int64_t i = 0; i < tile; i++) {
        const MsgVec v = msg_bytes_vec(m, gm, x, tile, i);
        if (!v.on) continue;
        CHECK(v.dst % 16 == 0 && v.dst >= dst && v.dst + 16 <= dst + (uint64_t)m.bytes);
        // the two aligned source granules the kernel loads both hold a byte of the message
        const uint64_t lo = v.src & ~(uint64_t)15, hi2 = (v.src + 15) & ~(uint64_t)15;
        CHECK(lo + 16 > src && hi2 < src + (uint64_t)m.bytes);
        for (int b = 0; b < 16; b++) put(out, v.dst + (uint64_t)b, v.src + (uint64_t)b);
      }
      if (x == 0)
        for (int64_t k = 0; k < gm.head; k++) put(out, dst + (uint64_t)k, src + (uint64_t)k);
      if (x == last)
        for (int64_t k = gm.ts; k < m.bytes; k++) put(out, dst + (uint64_t)k, src + (uint64_t)k);
      (void)lanes;
    } else {
      const uint32_t gl = m.g.glog;
      for (int64_t i = 0; i < tile; i++) {
        const uint64_t q = (uint64_t)x * (uint64_t)tile + (uint64_t)i;
        if (q >= m.g.ngran) continue;
        const uint64_t s = indexed_addr(m.g.s, (uint32_t)q, gl), d = indexed_addr(m.g.d, (uint32_t)q, gl);
        CHECK(s % ((uint64_t)1 << gl) == 0 && d % ((uint64_t)1 << gl) == 0);
        for (uint64_t b = 0; b < ((uint64_t)1 << gl); b++) put(out, d + b, s + b);
      }
    }
  }
}

// The message s -> d of n = s.total() bytes through the planner and the walk, against SideBytes::at
static void check_msgs(const std::vector<std::pair<SideBytes, SideBytes>>& msgs, int64_t tile, size_t want_tables = 0,
                       int64_t max_tiles = kMoveMaxTiles) {
  std::vector<MsgSeg> segs;
  std::string err;
  for (const auto& m : msgs) {
    if (m.first.total() <= 0) continue;
    MsgSeg sg{};
    const IdxEnt* st = m.first.irr ? m.first.irr->tab.data() : nullptr;
    const IdxEnt* dt = m.second.irr ? m.second.irr->tab.data() : nullptr;
    CHECK(plan_msg_seg(m.first, st, m.second, dt, &sg, &err) == kTypeOk);
    CHECK(sg.bytes == m.first.total());
    segs.push_back(sg);
  }
  std::vector<MsgsTable> tabs;
  plan_msgs_tables(segs, tile, &tabs, max_tiles);
  if (want_tables) CHECK(tabs.size() == want_tables);
  ByteMap got;
  for (const MsgsTable& t : tabs) {
    CHECK(t.n >= 1 && t.n <= kMsgsMax && t.tile0[0] == 0 && t.tile0[t.n] >= 1 && (int64_t)t.tile0[t.n] <= max_tiles);
    walk_table(t, tile, &got);
  }
  size_t total = 0;
  for (const auto& m : msgs) {
    const int64_t n = m.first.total();
    for (int64_t p = 0; p < n; p++) {
      auto it = got.find(m.second.at(p));
      CHECK(it != got.end() && it->second == m.first.at(p));
      if (it == got.end() || it->second != m.first.at(p)) return;
    }
    total += (size_t)(n > 0 ? n : 0);
  }
  CHECK(got.size() == total);  // nothing else is written: gaps and the rest of a longer receive layout stay
}

static void test_bytes_kind() {
  const int64_t lens[] = {0, 1, 15, 16, 17, 31, 33, 4099, 70001};
  const int al[5][2] = {{0, 0}, {0, 1}, {3, 3}, {5, 12}, {15, 8}};
  for (int64_t tile : {kStridedTile, kStridedTileNT})
    for (int64_t n : lens)
      for (auto& a : al) check_msgs({{run(0x100000 + (uint64_t)a[0], n), run(0x900000 + (uint64_t)a[1], n)}}, tile);
  // a message shorter than the receive run
  check_msgs({{run(0x100003, 33), run(0x900005, 4099)}}, kStridedTile);
  // a segment cut at max_tiles tiles
  check_msgs({{run(0x100005, 70001), run(0x90000c, 70001)}}, kStridedTile, 0, 2);
  MsgSeg one{};
  std::string err;
  CHECK(plan_msg_seg(run(0x1000, 64), nullptr, run(0x2000, 64), nullptr, &one, &err) == kTypeOk && one.kind == kMsgBytes);
}

static SideBytes regular(uint64_t base, int64_t bb, int64_t sb, int64_t nb, int64_t eb, int64_t items) {
  SideBytes x;
  x.base = base;
  x.bb = bb;
  x.sb = sb;
  x.nb = nb;
  x.eb = eb;
  x.items = items;
  return x;
}

static SideBytes irregular(uint64_t base, const std::vector<ElemBlock>& v, int bsz, int64_t items) {
  TypeForm old = contiguous_form(1, bsz, 1), f;
  int64_t lb = v[0].off, ub = v[0].off + v[0].len;
  for (const ElemBlock& b : v) lb = std::min(lb, b.off), ub = std::max(ub, b.off + b.len);
  normal_form(old, v, lb, ub, false, false, &f);
  f.code = kDerivedBase + 1;
  SideBytes x;
  std::string err;
  CHECK(plan_side(f, base, items, 0, &x, &err));
  return x;
}

static void test_granule_kind() {
  // one-granule blocks at each granule size 1..16 B: the granule is the largest power of two dividing g
  for (int64_t g = 1; g <= 16; g++) {
    const SideBytes s = regular(0x100000, g, 3 * g, 37, 37 * 3 * g, 3), d = run(0x900000, 37 * 3 * g);
    MsgSeg m{};
    std::string err;
    CHECK(plan_msg_seg(s, nullptr, d, nullptr, &m, &err) == kTypeOk && m.kind == kMsgGranule);
    CHECK(((int64_t)1 << m.g.glog) == (g & -g));
    check_msgs({{s, d}}, kStridedTile);
    check_msgs({{d, s}}, kStridedTileNT);
  }
  // a 3-block and a 513-block irregular table, as source, as destination and against each other
  std::vector<ElemBlock> b3 = {{7, 3}, {0, 2}, {20, 5}}, b513;
  for (int i = 0; i < 513; i++) b513.push_back(ElemBlock{(int64_t)((i * 7) % 513) * 4 + 1, 1 + i % 3});
  int64_t n513 = 0;
  for (auto& b : b513) n513 += b.len;
  for (int bsz : {1, 8}) {
    const SideBytes i3 = irregular(0x100000, b3, bsz, 5), c3 = run(0x900000, 5 * 10 * bsz);
    check_msgs({{i3, c3}}, kStridedTile);
    check_msgs({{c3, i3}}, kStridedTile);
    const SideBytes i513 = irregular(0x200000, b513, bsz, 2), c513 = run(0xa00000 + (uint64_t)bsz, 2 * n513 * bsz);
    check_msgs({{i513, c513}}, kStridedTile);
    check_msgs({{c513, i513}}, kStridedTileNT);
    // irregular to irregular: 2 * n513 elements into a layout of 3-block items, the last item part-filled
    const int64_t items = (2 * n513 + 9) / 10;
    const SideBytes big3 = irregular(0x4000000, b3, bsz, items);
    check_msgs({{i513, big3}}, kStridedTile);
  }
}

static void test_tables() {
  // mixed kinds in one table; a batch that closes a table exactly at kMsgsMax, and one at kMsgsMax + 1
  for (int n : {kMsgsMax, kMsgsMax + 1, 2 * kMsgsMax + 1}) {
    std::vector<std::pair<SideBytes, SideBytes>> msgs;
    for (int i = 0; i < n; i++) {
      const uint64_t sb = 0x100000 + (uint64_t)i * 0x10000, db = 0x9000000 + (uint64_t)i * 0x10000;
      if (i % 3 == 0) msgs.push_back({run(sb + (uint64_t)(i % 16), 100 + i), run(db + (uint64_t)((5 * i) % 16), 100 + i)});
      else if (i % 3 == 1) msgs.push_back({regular(sb, 8, 272, 32, 8, 1), run(db + 8, 256)});
      else msgs.push_back({run(sb, 96), regular(db, 4, 12, 24, 4, 1)});
    }
    check_msgs(msgs, kStridedTile, (size_t)((n + kMsgsMax - 1) / kMsgsMax));
  }
  static_assert(sizeof(MsgsTable) <= 4096, "kernel argument");
  CHECK(kMsgsMax >= 8);  // a 2-D halo's eight messages fit one launch
}

// --cases: one case of tests/msgs_cases.py per line of stdin, the send side and then the receive side, each
//   C | V <count> <blocklength> <stride> | I <n> <n blocklengths> <n displacements>
//   <items> <byte offset of the buffer position>
// over MPI.BYTE, planned over two 16-byte aligned buffers through plan_side and plan_msg_seg as the transport does.
// Prints per case
//   kind glog stab dtab ngran bytes sh da tiles tiles_nt transpose slo shi dlo dhi
// (stab, dtab: the side has a block table; sh, da: (src - dst) & 15 and dst & 15, of a bytes segment; tiles at
// kStridedTile and at kStridedTileNT; transpose: what plan_transpose_seg says; lo, hi: the bytes of its buffer
// a layout touches). A message of up to 4 KiB is walked at both tiles, as above.
static bool read_side(uint64_t buf, SideBytes* out) {
  using V = std::vector<int64_t>;
  char ctor;
  long long v, n = 0;
  if (!(std::cin >> ctor)) return false;
  TypeForm b, f;
  std::string err;
  CHECK(basic_form(1, &b));
  f = b;
  if (ctor == 'V') {
    long long a[3];
    if (!(std::cin >> a[0] >> a[1] >> a[2])) return false;
    CHECK(vector_form(a[0], a[1], a[2], b, &f, &err) == kTypeOk);
  } else if (ctor == 'I') {
    if (!(std::cin >> n) || n < 1 || n > (1 << 20)) return false;
    V a;
    for (long long i = 0; i < 2 * n && (std::cin >> v); i++) a.push_back(v);
    if ((long long)a.size() != 2 * n) return false;
    CHECK(indexed_form(n, a.data(), a.data() + n, b, &f, &err) == kTypeOk);
    f.code = kDerivedBase + 1;
  } else if (ctor != 'C') {
    return false;
  }
  long long items, off;
  if (!(std::cin >> items >> off) || items < 1 || off < 0) return false;
  CHECK(plan_side(f, buf + (uint64_t)off, items, 0, out, &err));
  return true;
}

static int run_cases() {
  const uint64_t sbuf = 0x10000000, dbuf = 0x40000000;
  int n = 0;
  while (std::cin >> std::ws && std::cin.peek() != EOF) {
    SideBytes s, d;
    if (!read_side(sbuf, &s) || !read_side(dbuf, &d) || s.total() <= 0 || d.total() < s.total()) {
      printf("case %d: malformed\n", n);
      return 2;
    }
    MsgSeg m{};
    std::string err;
    const IdxEnt* st = s.irr ? s.irr->tab.data() : nullptr;
    const IdxEnt* dt = d.irr ? d.irr->tab.data() : nullptr;
    CHECK(plan_msg_seg(s, st, d, dt, &m, &err) == kTypeOk);
    CHECK(m.bytes == s.total());
    TransposeSeg ts;
    const bool tr = plan_transpose_seg(s, d, &ts);
    if (m.bytes <= 4096)
      for (int64_t tile : {kStridedTile, kStridedTileNT}) check_msgs({{s, d}}, tile, 1);
    uint64_t slo, shi, dlo, dhi;
    s.span(&slo, &shi);
    d.span(&dlo, &dhi);
    const bool by = m.kind == kMsgBytes;
    printf("%u %u %d %d %u %lld %u %u %lld %lld %d %lld %lld %lld %lld\n", m.kind, by ? 0u : m.g.glog,
           !by && m.g.s.tab ? 1 : 0, !by && m.g.d.tab ? 1 : 0, by ? 0u : m.g.ngran, (long long)m.bytes,
           by ? (unsigned)((m.g.s.r.base - m.g.d.r.base) & 15u) : 0u, by ? (unsigned)(m.g.d.r.base & 15u) : 0u,
           (long long)msg_tiles(m, kStridedTile), (long long)msg_tiles(m, kStridedTileNT), tr ? 1 : 0,
           (long long)(slo - sbuf), (long long)(shi - sbuf), (long long)(dlo - dbuf), (long long)(dhi - dbuf));
    n++;
  }
  if (g_fail) {
    printf("msgs_plan_test: %d FAILED\n", g_fail);
    return 1;
  }
  printf("msgs_plan_test: ok (%d cases)\n", n);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "--cases") return run_cases();
  test_bytes_kind();
  test_granule_kind();
  test_tables();
  if (g_fail) {
    printf("msgs_plan_test: %d FAILED\n", g_fail);
    return 1;
  }
  printf("msgs_plan_test: ok\n");
  return 0;
}
