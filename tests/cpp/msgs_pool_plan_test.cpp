// CPU test of k_msgs_pool's launch index (mpjexpress_amd/csrc/mpjx_msgs_pool_plan.hpp) and of the per-lane mapping
// it shares with k_msgs (mpjx_msgs_plan.hpp): plain C++17, no HIP. A pool is an array of segments on the host;
// every packed byte of every message is walked, block by block and lane by lane as the kernel does it, against
// SideBytes::at. Built by the Makefile with g++, and by tests/test_preq_abi.py under the sanitizers.
#include <stdio.h>
#include <string.h>

#include <map>

#include "../../mpjexpress_amd/csrc/mpjx_msgs_pool_plan.hpp"

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

// What k_msgs_pool does with one index over `pool`, as a map destination byte -> source byte; every destination
// byte at most once (CHECKed)
using ByteMap = std::map<uint64_t, uint64_t>;
static void put(ByteMap* m, uint64_t d, uint64_t s) { CHECK(m->emplace(d, s).second); }

static void walk_index(const std::vector<MsgSeg>& pool, const MsgsIndex& ix, int64_t tile, ByteMap* out) {
  for (uint32_t g = 0; g < ix.tile0[ix.n]; g++) {
    int c = 0, hi = ix.n;
    while (hi - c > 1) {
      const int mid = (c + hi) >> 1;
      if (ix.tile0[mid] <= g) c = mid;
      else hi = mid;
    }
    CHECK(ix.tile0[c] <= g && g < ix.tile0[c + 1]);
    CHECK(ix.slot[c] < pool.size());
    const MsgSeg& m = pool[ix.slot[c]];
    const int64_t x = g - ix.tile0[c], last = (int64_t)(ix.tile0[c + 1] - ix.tile0[c]) - 1;
    CHECK(last + 1 == msg_tiles(m, tile));  // the index's tiles are the segment's for this tile size
    if (m.kind == kMsgBytes) {
      const uint64_t src = m.g.s.r.base, dst = m.g.d.r.base;
      const MoveGeom gm = move_geom(dst, m.bytes);
      for (int64_t i = 0; i < tile; i++) {
        const MsgVec v = msg_bytes_vec(m, gm, x, tile, i);
        if (!v.on) continue;
        CHECK(v.dst % 16 == 0 && v.dst >= dst && v.dst + 16 <= dst + (uint64_t)m.bytes);
        const uint64_t lo = v.src & ~(uint64_t)15, hi2 = (v.src + 15) & ~(uint64_t)15;
        CHECK(lo + 16 > src && hi2 < src + (uint64_t)m.bytes);
        for (int b = 0; b < 16; b++) put(out, v.dst + (uint64_t)b, v.src + (uint64_t)b);
      }
      if (x == 0)
        for (int64_t k = 0; k < gm.head; k++) put(out, dst + (uint64_t)k, src + (uint64_t)k);
      if (x == last)
        for (int64_t k = gm.ts; k < m.bytes; k++) put(out, dst + (uint64_t)k, src + (uint64_t)k);
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

using Msgs = std::vector<std::pair<SideBytes, SideBytes>>;

// The messages go into a PoolMap and a host pool as a communicator stores them, every second slot left to
// another pair so that slots and batch positions differ; then the whole set is one batch in REVERSE order (a
// batch is any subset in any order), planned and walked.
static void check_pool(const Msgs& msgs, int64_t tile, size_t want_indices = 0, int64_t max_tiles = kMoveMaxTiles,
                       int batch_max = kPoolBatchMax) {
  PoolMap pm;
  std::vector<MsgSeg> pool((size_t)kPoolSlots);
  std::string err;
  std::vector<PoolRef> refs;
  uint64_t serial = 1;
  std::vector<std::pair<uint64_t, uint64_t>> keys;
  for (const auto& m : msgs) {
    MsgSeg sg{};
    const IdxEnt* st = m.first.irr ? m.first.irr->tab.data() : nullptr;
    const IdxEnt* dt = m.second.irr ? m.second.irr->tab.data() : nullptr;
    CHECK(plan_msg_seg(m.first, st, m.second, dt, &sg, &err) == kTypeOk);
    CHECK(sg.bytes == m.first.total());
    if (keys.size() % 2 == 1) CHECK(pm.put(serial + 2, serial + 3, sg, nullptr, nullptr) >= 0 || pm.in_use() == kPoolSlots);
    const int slot = pm.put(serial, serial + 1, sg, nullptr, nullptr);
    CHECK(slot >= 0 && slot < kPoolSlots);
    if (slot < 0) return;
    pool[(size_t)slot] = sg;
    keys.emplace_back(serial, serial + 1);
    serial += 4;
  }
  for (auto it = keys.rbegin(); it != keys.rend(); ++it) {
    const PoolMap::Entry* e = pm.find(it->first, it->second);
    CHECK(e != nullptr);
    if (!e) return;
    refs.push_back(PoolRef{e->slot, tile == kStridedTile ? e->tiles : e->tiles_nt});
  }
  std::vector<MsgsIndex> ixs;
  plan_msgs_indices(refs, &ixs, max_tiles, batch_max);
  if (want_indices) CHECK(ixs.size() == want_indices);
  ByteMap got;
  size_t entries = 0;
  for (const MsgsIndex& ix : ixs) {
    CHECK(ix.n >= 1 && ix.n <= batch_max && ix.tile0[0] == 0 && ix.tile0[ix.n] >= 1 && (int64_t)ix.tile0[ix.n] <= max_tiles);
    for (int c = 0; c < ix.n; c++) CHECK(ix.tile0[c + 1] > ix.tile0[c]);
    entries += (size_t)ix.n;
    walk_index(pool, ix, tile, &got);
  }
  CHECK(entries == msgs.size());
  size_t total = 0;
  for (const auto& m : msgs) {
    const int64_t n = m.first.total();
    for (int64_t p = 0; p < n; p++) {
      auto it = got.find(m.second.at(p));
      CHECK(it != got.end() && it->second == m.first.at(p));
      if (it == got.end() || it->second != m.first.at(p)) return;
    }
    total += (size_t)n;
  }
  CHECK(got.size() == total);  // nothing else is written
}

// n small messages of mixed kinds, each of one tile
static Msgs small_msgs(int n) {
  Msgs msgs;
  for (int i = 0; i < n; i++) {
    const uint64_t sb = 0x100000 + (uint64_t)i * 0x1000, db = 0x9000000 + (uint64_t)i * 0x1000;
    if (i % 3 == 0) msgs.push_back({run(sb + (uint64_t)(i % 16), 20 + i % 50), run(db + (uint64_t)((5 * i) % 16), 20 + i % 50)});
    else if (i % 3 == 1) msgs.push_back({regular(sb, 8, 272, 8, 8, 1), run(db + 8, 64)});
    else msgs.push_back({run(sb, 48), regular(db, 4, 12, 12, 4, 1)});
  }
  return msgs;
}

static void test_index_sizes() {
  static_assert(sizeof(MsgsIndex) < 4096 && kPoolBatchMax == 512 && kPoolSlots > kPoolBatchMax, "index");
  static_assert(sizeof(PoolPut) + sizeof(void*) <= 4096, "put argument");
  for (int64_t tile : {kStridedTile, kStridedTileNT}) {
    for (int n : {1, 2, 24, 25}) check_pool(small_msgs(n), tile, 1);
    // 512 fill one index exactly; 513 give two
    check_pool(small_msgs(512), tile, 1);
    check_pool(small_msgs(513), tile, 2);
  }
  // the empty batch
  std::vector<MsgsIndex> ixs;
  plan_msgs_indices({}, &ixs);
  CHECK(ixs.empty());
}

static void test_tiles() {
  for (int64_t tile : {kStridedTile, kStridedTileNT}) {
    // bytes kind: one tile and several, at alignment pairs; 16 KiB + 48 B at (1, 2) is two tiles of 1024 vectors
    const int64_t lens[] = {1, 15, 16, 17, 33, 4099, 16 * 1024 + 48, 70001};
    const int al[4][2] = {{0, 0}, {1, 2}, {5, 12}, {15, 8}};
    for (int64_t n : lens)
      for (auto& a : al) check_pool({{run(0x100000 + (uint64_t)a[0], n), run(0x900000 + (uint64_t)a[1], n)}}, tile);
    MsgSeg two = msg_bytes_seg(0x100001, 0x900002, 16 * 1024 + 48);
    CHECK(msg_tiles(two, kStridedTile) == 2);
    // a message shorter than the receive run
    check_pool({{run(0x100003, 33), run(0x900005, 4099)}}, tile);
    // granule kind at every granule size, 37 granules (one tile) and 1025 granules (two tiles of 1024 / three of 512)
    for (int64_t g = 1; g <= 16; g <<= 1)
      for (int64_t nb : {(int64_t)37, (int64_t)1025}) {
        const SideBytes s = regular(0x100000, g, 3 * g, nb, nb * 3 * g, 1), d = run(0x900000, nb * g);
        MsgSeg m{};
        std::string err;
        CHECK(plan_msg_seg(s, nullptr, d, nullptr, &m, &err) == kTypeOk && m.kind == kMsgGranule);
        CHECK(((int64_t)1 << m.g.glog) == g && (int64_t)m.g.ngran == nb);
        CHECK(msg_tiles(m, tile) == (nb + tile - 1) / tile);
        check_pool({{s, d}}, tile);
        check_pool({{d, s}}, tile);
      }
  }
  // irregular sides
  std::vector<ElemBlock> b3 = {{7, 3}, {0, 2}, {20, 5}}, b513;
  for (int i = 0; i < 513; i++) b513.push_back(ElemBlock{(int64_t)((i * 7) % 513) * 4 + 1, 1 + i % 3});
  int64_t n513 = 0;
  for (auto& b : b513) n513 += b.len;
  for (int bsz : {1, 8}) {
    const SideBytes i3 = irregular(0x100000, b3, bsz, 5), c3 = run(0x900000, 5 * 10 * bsz);
    const SideBytes i513 = irregular(0x200000, b513, bsz, 2), c513 = run(0xa00000 + (uint64_t)bsz, 2 * n513 * bsz);
    check_pool({{i3, c3}, {c513, i513}}, kStridedTile, 1);
    check_pool({{i513, c513}, {c3, i3}}, kStridedTileNT, 1);
  }
}

static void test_splits() {
  // mixed one-tile and several-tile entries, closed by the tile limit and by the entry limit
  Msgs msgs = small_msgs(7);
  msgs.push_back({run(0x5000003, 70001), run(0x6000005, 70001)});  // 5 tiles of 1024 vectors
  msgs.push_back({run(0x7000000, 40), run(0x8000000, 40)});
  check_pool(msgs, kStridedTile, 1);
  check_pool(msgs, kStridedTile, 0, 5);            // no index above 5 tiles
  check_pool(msgs, kStridedTile, 3, kMoveMaxTiles, 4);  // 9 entries, 4 per index
  std::vector<PoolRef> refs = {{3, 2}, {9, 5}, {1, 1}, {4, 4}, {7, 1}};
  std::vector<MsgsIndex> ixs;
  plan_msgs_indices(refs, &ixs, 7);
  CHECK(ixs.size() == 2);
  if (ixs.size() == 2) {
    CHECK(ixs[0].n == 2 && ixs[0].slot[0] == 3 && ixs[0].slot[1] == 9 && ixs[0].tile0[1] == 2 && ixs[0].tile0[2] == 7);
    CHECK(ixs[1].n == 3 && ixs[1].slot[0] == 1 && ixs[1].slot[1] == 4 && ixs[1].slot[2] == 7 && ixs[1].tile0[3] == 6);
  }
  plan_msgs_indices(refs, &ixs, 5);
  CHECK(ixs.size() == 4 && ixs[0].n == 1 && ixs[1].n == 1 && ixs[2].n == 2 && ixs[3].n == 1);
}

int main() {
  test_index_sizes();
  test_tiles();
  test_splits();
  if (g_fail) {
    printf("msgs_pool_plan_test: %d FAILED\n", g_fail);
    return 1;
  }
  printf("msgs_pool_plan_test: ok\n");
  return 0;
}
