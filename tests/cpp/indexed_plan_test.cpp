// indexed_plan_test.cpp — the irregular datatypes' forms, the planner of k_indexed and its address function
// (mpjexpress_amd/csrc/mpjx_indexed_plan.hpp) on the CPU. A stand-alone program: plain g++, no HIP;
// tests/test_indexed_abi.py builds it with -fsanitize=address,undefined.
//   - forms: the reference's cases (Indexed.java, hvec.java), merging, normalisation to the regular form,
//     flattening of a non-contiguous oldtype, bounds with lb > 0, the errors
//   - for EVERY granule of a set of segments (irregular x irregular, irregular x regular, irregular x
//     contiguous; tables of 1, 2, 3, 1,000 and 5,000 blocks; granules 1..16 B; items 0 / 1 / 3) the kernel's
//     address function against a brute-force walk of the block list, tile by tile as the kernel's lanes go
//   - the granule choice, launch-table planning, and the overlap sweep on irregular layouts
#include <stdio.h>

#include <numeric>
#include <random>

#include "../../mpjexpress_amd/csrc/mpjx_indexed_plan.hpp"

using namespace mpjx;

static int failures = 0;
#define EXPECT(cond)                                         \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                            \
    }                                                        \
  } while (0)

using V = std::vector<int64_t>;

static TypeForm basic(int code) {
  TypeForm f;
  EXPECT(basic_form(code, &f));
  return f;
}
static TypeForm indexed(const V& bl, const V& d, const TypeForm& old, int want = kTypeOk, bool h = false) {
  TypeForm f;
  std::string err;
  const int rc = (h ? hindexed_form : indexed_form)((int64_t)bl.size(), bl.data(), d.data(), old, &f, &err);
  EXPECT(rc == want);
  EXPECT((rc == kTypeOk) == err.empty());
  return f;
}
static TypeForm hvector(int64_t c, int64_t b, int64_t s, const TypeForm& old, int want = kTypeOk) {
  TypeForm f;
  std::string err;
  EXPECT(hvector_form(c, b, s, old, &f, &err) == want);
  return f;
}
static TypeForm vec(int64_t c, int64_t b, int64_t s, const TypeForm& old) {
  TypeForm f;
  std::string err;
  EXPECT(vector_form(c, b, s, old, &f, &err) == kTypeOk);
  return f;
}
// (offset, length) of the merged blocks in base elements
static std::vector<std::pair<int64_t, int64_t>> blocks(const TypeForm& f) {
  std::vector<std::pair<int64_t, int64_t>> v;
  for (int64_t b = 0; b < form_nblocks(f); b++) {
    int64_t o, l;
    form_block(f, b, &o, &l);
    v.push_back({o, l});
  }
  return v;
}
using B = std::vector<std::pair<int64_t, int64_t>>;

static void test_forms() {
  const TypeForm I = basic(5), D = basic(8), D2 = basic(0x108);
  TypeForm a = indexed({3, 1, 0, 2}, {7, 0, 4, 12}, I);
  EXPECT(a.irr && a.size() == 6 && a.lb() == 0 && a.ub() == 14 && a.extent() == 14);
  EXPECT((blocks(a) == B{{7, 3}, {0, 1}, {12, 2}}));  // pack order, the empty block dropped
  EXPECT(!a.irr->self_overlap && a.irr->amask % 4 == 0 && (a.irr->amask & 4));
  TypeForm b = indexed({2, 1}, {9, 4}, I);
  EXPECT(b.irr && b.lb() == 4 && b.ub() == 11 && b.extent() == 7 && b.size() == 3);
  // Indexed over a pair type counts in pairs; Hindexed gives the offsets in base elements
  TypeForm p = indexed({2, 1}, {9, 4}, D2), q = indexed({2, 1}, {18, 8}, D2, kTypeOk, true);
  EXPECT(p.irr && q.irr && blocks(p) == blocks(q) && (blocks(p) == B{{18, 4}, {8, 2}}));
  EXPECT(p.lb() == 8 && p.ub() == 22 && p.size() == 6 && p.base == 8 && p.bsz == 8);
  // the reference's upper triangle: row i has 8 - i elements from column i of an 8 x 8 matrix
  V tl, td;
  for (int i = 0; i < 8; i++) tl.push_back(8 - i), td.push_back(9 * i);
  TypeForm tri = indexed(tl, td, D);
  EXPECT(tri.irr && tri.size() == 36 && form_nblocks(tri) == 8 && tri.lb() == 0 && tri.ub() == 64);
  // abutting blocks merge, in pack order AND address order only
  EXPECT((blocks(indexed({2, 3, 1}, {0, 2, 9}, I)) == B{{0, 5}, {9, 1}}));
  EXPECT((blocks(indexed({2, 2}, {2, 0}, I)) == B{{2, 2}, {0, 2}}));
  // a regular list IS the Vector
  TypeForm r = indexed({2, 2, 2}, {0, 5, 10}, I), v = vec(3, 2, 5, I);
  EXPECT(!r.irr && r.nblocks == v.nblocks && r.blocklen == v.blocklen && r.stride == v.stride && r.extent() == v.extent());
  TypeForm c = indexed({2, 2}, {0, 2}, I);
  EXPECT(!c.irr && c.contiguous() && c.size() == 4);
  EXPECT(indexed({2, 2}, {1, 6}, I).irr);  // the same shape one element in is not: lb = 1
  // one block with lb > 0: Indexed([2],[3],INT) has lb 3, extent 2
  TypeForm one = indexed({2}, {3}, I);
  EXPECT(one.irr && one.lb() == 3 && one.ub() == 5 && one.extent() == 2 && form_nblocks(one) == 1);
  // hvec.java: Hvector(3, 1, ext + off, Vector(2, 3, 4, INT)), ext = 7
  const TypeForm v234 = vec(2, 3, 4, I);
  TypeForm h0 = hvector(3, 1, 7, v234), h1 = hvector(3, 1, 8, v234), h2 = hvector(3, 1, 9, v234), hm = hvector(3, 1, 6, v234);
  EXPECT((blocks(h0) == B{{0, 3}, {4, 6}, {11, 6}, {18, 3}}) && h0.extent() == 21 && h0.size() == 18);
  EXPECT(!h1.irr && h1.nblocks == 6 && h1.blocklen == 3 && h1.stride == 4 && h1.extent() == 23);
  EXPECT(h2.irr && form_nblocks(h2) == 6 && h2.extent() == 25 && !h2.irr->self_overlap);
  EXPECT(hm.irr && hm.size() == 18 && hm.extent() == 19 && hm.irr->self_overlap);  // [4,7) and [6,9) share element 6
  // an irregular oldtype is flattened; blocklength counts ITEMS of it, its extent apart
  TypeForm nest = indexed({2, 1}, {0, 3}, b);  // b: (9,2) (4,1), lb 4, extent 7
  EXPECT((blocks(nest) == B{{9, 2}, {4, 1}, {16, 2}, {11, 1}, {30, 2}, {25, 1}}) && nest.lb() == 4 && nest.ub() == 32);
  // empty types
  for (const TypeForm& e : {indexed({}, {}, I), indexed({0, 0}, {5, 9}, I), hvector(0, 3, 2, I), hvector(4, 0, 2, I)})
    EXPECT(!e.irr && e.size() == 0 && e.extent() == 0 && e.lb() == 0 && e.ub() == 0);
  // errors
  indexed({2, -1}, {0, 4}, I, kTypeErrArg);
  indexed({1, 1}, {3, -1}, I, kTypeErrUnsupported);
  indexed({0}, {-5}, I);  // a zero-length block takes no part
  hvector(-1, 1, 2, I, kTypeErrArg);
  hvector(2, -1, 2, I, kTypeErrArg);
  hvector(2, 1, 0, I, kTypeErrUnsupported);
  hvector(2, 1, -3, I, kTypeErrUnsupported);
  hvector(1, 1, -3, I);
  indexed({(int64_t)1 << 61}, {0}, D, kTypeErrArg);
  indexed({1}, {(int64_t)1 << 61}, D, kTypeErrArg);
  TypeForm f;
  std::string err;
  EXPECT(indexed_form(-1, nullptr, nullptr, I, &f, &err) == kTypeErrArg && err.find("-1") != std::string::npos);
  EXPECT(indexed_form(2, nullptr, nullptr, I, &f, &err) == kTypeErrArg && err.find("NULL") != std::string::npos);
  // the block bound: 2^20 unit blocks are a type, one more is not; a huge run of a contiguous old is one block
  V ones((size_t)kIndexedMaxBlocks + 1, 1), ev(ones.size());
  for (size_t i = 0; i < ev.size(); i++) ev[i] = 2 * (int64_t)i + (i > 0);
  EXPECT(indexed_form(kIndexedMaxBlocks + 1, ones.data(), ev.data(), basic(1), &f, &err) == kTypeErrUnsupported);
  EXPECT(err.find("1048576") != std::string::npos);
  EXPECT(indexed_form(kIndexedMaxBlocks, ones.data(), ev.data(), basic(1), &f, &err) == kTypeOk && f.irr);
  EXPECT(form_nblocks(indexed({(int64_t)1 << 40, 1}, {1, 0}, I)) == 2);
  const TypeForm run = hvector((int64_t)1 << 40, 3, 3, basic(1));  // abutting blocks of a contiguous old: one run
  EXPECT(!run.irr && run.contiguous() && run.size() == 3 * ((int64_t)1 << 40));
  hvector((int64_t)1 << 40, 1, (int64_t)1 << 40, D, kTypeErrArg);
  hvector((int64_t)1 << 40, 1, 2, basic(1), kTypeErrUnsupported);
  EXPECT(hvector((int64_t)1 << 20, 1, 30, v234, kTypeErrUnsupported).size() == 0);  // ends at the bound, not after 2^31 pushes
}

// ---- the address function against a walk of the block list -------------------------------------------------

// Every byte address of a layout in packed order, from the rules alone
static std::vector<uint64_t> walk(const TypeForm& f, uint64_t buf, int64_t count, int64_t disp) {
  std::vector<uint64_t> out;
  const uint64_t origin = buf + (uint64_t)(disp * f.bsz);
  for (int64_t k = 0; k < count; k++)
    for (const auto& b : blocks(f))
      for (int64_t w = 0; w < b.second * f.bsz; w++) out.push_back(origin + (uint64_t)((k * f.extent() + b.first) * f.bsz + w));
  return out;
}

// Plan s -> d, then take every granule of the segment through indexed_addr in the kernel's lane order
static void check_seg(const TypeForm& sf, int64_t sc, int64_t sd, const TypeForm& df, int64_t dc, int64_t dd,
                      uint32_t want_glog, uint64_t sbuf = 0x10000, uint64_t dbuf = 0x900000) {
  SideBytes s, d;
  std::string err;
  EXPECT(plan_side(sf, sbuf, sc, sd, &s, &err) && plan_side(df, dbuf, dc, dd, &d, &err));
  const std::vector<uint64_t> sw = walk(sf, sbuf, sc, sd), dw = walk(df, dbuf, dc, dd);
  EXPECT(sw.size() == dw.size() && (int64_t)sw.size() == s.total() && s.total() == d.total());
  for (int64_t p = 0; p < s.total(); p += 7) EXPECT(s.at(p) == sw[(size_t)p] && d.at(p) == dw[(size_t)p]);
  if (s.total() == 0) return;
  uint64_t lo, hi;
  s.span(&lo, &hi);
  EXPECT(lo == *std::min_element(sw.begin(), sw.end()) && hi == *std::max_element(sw.begin(), sw.end()) + 1);
  IndexedSeg sg;
  // the "device" tables are the host lists: the host build of idx_entry reads them in place
  EXPECT(plan_indexed_seg(s, s.irr ? s.irr->tab.data() : nullptr, d, d.irr ? d.irr->tab.data() : nullptr, &sg, &err) == kTypeOk);
  if (sg.glog != want_glog) printf("glog %u, wanted %u (total %lld)\n", sg.glog, want_glog, (long long)s.total());
  EXPECT(sg.glog == want_glog && ((uint64_t)sg.ngran << sg.glog) == (uint64_t)s.total());
  EXPECT((sg.s.tab != nullptr) == (s.irr != nullptr) && (sg.d.tab != nullptr) == (d.irr != nullptr));
  const uint32_t g = 1u << sg.glog;
  for (int64_t gran : {kStridedTile, kStridedTileNT}) {
    const int64_t lanes = gran == kStridedTile ? 256 : 512, tiles = strided_tiles(sg.ngran, gran);
    uint64_t seen = 0;
    for (int64_t x = 0; x < tiles; x++)
      for (int64_t u = 0; u < gran / lanes; u++)
        for (int64_t t = 0; t < lanes; t++) {
          const uint64_t q = (uint64_t)x * gran + u * lanes + t;
          if (q >= sg.ngran) continue;
          const uint64_t a = indexed_addr(sg.s, (uint32_t)q, sg.glog), b = indexed_addr(sg.d, (uint32_t)q, sg.glog);
          bool ok = a % g == 0 && b % g == 0;
          for (uint32_t w = 0; ok && w < g; w++) ok = sw[q * g + w] == a + w && dw[q * g + w] == b + w;  // none straddles a block
          if (!ok) {
            printf("granule %llu: src %#llx dst %#llx\n", (unsigned long long)q, (unsigned long long)a, (unsigned long long)b);
            EXPECT(ok);
            return;
          }
          seen++;
        }
    EXPECT(seen == sg.ngran);
  }
}

static TypeForm permutation(int n, int unit, const TypeForm& old, unsigned seed, bool ragged) {
  std::vector<int> order((size_t)n);
  std::iota(order.begin(), order.end(), 0);
  std::shuffle(order.begin(), order.end(), std::mt19937(seed));
  V bl, d;
  for (int i : order) bl.push_back(ragged ? unit * (1 + i % 3) : unit), d.push_back((int64_t)i * unit * 4);
  return indexed(bl, d, old);
}

static void test_addresses() {
  const TypeForm Bt = basic(1), C = basic(2), I = basic(5), D = basic(8), D2 = basic(0x108);
  const TypeForm a = indexed({3, 1, 2}, {8, 0, 4}, I), h = indexed({2, 2, 2}, {1, 9, 4}, I, kTypeOk, true);
  for (int64_t items : {0, 1, 3})
    for (int64_t off : {0, 1}) {
      check_seg(a, items, off, h, items, off, 2);                     // irregular x irregular, different blocking
      check_seg(a, items, off, vec(2, 3, 4, I), items, 1 - off, 2);   // irregular x regular
      check_seg(I, 6 * items, off, h, items, off, 2);                 // contiguous x irregular
      check_seg(indexed({2}, {3}, I), items, off, I, 2 * items, 0, off ? 3 : 2);  // one block, lb 3: a contiguous side at +12 / +16
    }
  check_seg(indexed({2, 1}, {3, 0}, Bt), 3, 1, Bt, 9, 0, 0);  // 2 blocks, granule 1
  check_seg(indexed({2, 4}, {6, 0}, C), 3, 1, C, 18, 1, 1);   // granule 2
  check_seg(indexed({2, 4}, {6, 0}, I), 3, 2, I, 18, 2, 3);   // INT blocks and offsets that give granule 8 ...
  check_seg(indexed({4, 8}, {12, 0}, I), 3, 4, I, 36, 0, 4);  // ... and 16
  check_seg(indexed({4, 8}, {12, 0}, I), 3, 1, I, 36, 0, 2);  // the buffer one element in: 4
  check_seg(indexed({1, 2}, {3, 0}, D2), 3, 0, D, 18, 0, 4);
  check_seg(indexed({1, 2}, {3, 0}, D), 3, 0, D, 9, 0, 3);
  // 1,000 unit BYTE blocks x 3 items: granule 1, three tiles, tiles crossing items
  check_seg(permutation(1000, 1, Bt, 1, false), 3, 1, Bt, 3000, 3, 0);
  check_seg(Bt, 3000, 3, permutation(1000, 1, Bt, 2, false), 3, 1, 0);
  check_seg(permutation(5000, 1, I, 5, false), 3, 0, permutation(1000, 5, I, 6, false), 3, 1, 2);  // 5,000 x 1,000 blocks
  check_seg(permutation(5000, 2, I, 7, true), 1, 2, I, 20000 - 2, 0, 3);
}

static void test_tables_and_granule() {
  const TypeForm I = basic(5);
  SideBytes s, d;
  std::string err;
  const TypeForm a = indexed({3, 1, 2}, {8, 0, 4}, I);
  EXPECT(plan_side(a, 0x1000, 5, 0, &s, &err) && plan_side(I, 0x8000, 30, 0, &d, &err));
  EXPECT(s.irr && s.nb == 3 && s.items == 5 && s.eb == 44 && s.total() == 120 && s.blocks() == 15 && !s.contiguous());
  IndexedSeg sg;
  EXPECT(plan_indexed_seg(s, s.irr->tab.data(), d, nullptr, &sg, &err) == kTypeOk && sg.ngran == 30 && sg.glog == 2);
  EXPECT(sg.s.r.bbg.d == 6 && sg.s.r.nb.d == 3 && sg.s.r.eb == 44 && sg.d.tab == nullptr);
  std::vector<IndexedSeg> segs(2 * kIndexedMax + 3, sg);
  segs[5].ngran = 0;  // an empty segment takes no slot
  std::vector<IndexedTable> tabs;
  plan_indexed_tables(segs, kStridedTile, &tabs);
  EXPECT(tabs.size() == 3 && tabs[0].n == kIndexedMax && tabs[1].n == kIndexedMax && tabs[2].n == 2);
  EXPECT(tabs[0].tile0[kIndexedMax] == (uint32_t)kIndexedMax && tabs[2].tile0[2] == 2);
  sg.ngran = 5000;
  plan_indexed_tables({sg, sg}, kStridedTileNT, &tabs);
  EXPECT(tabs.size() == 1 && tabs[0].tile0[1] == 10 && tabs[0].tile0[2] == 20);
  plan_indexed_tables({sg, sg, sg}, kStridedTileNT, &tabs, 25);  // a table closes at max_tiles too
  EXPECT(tabs.size() == 2 && tabs[0].n == 2 && tabs[1].n == 1);
  // 2^32 granules or more in one segment are unsupported: a one-byte granule over 4 GiB + 3 bytes
  const TypeForm big = indexed({1, ((int64_t)1 << 32) + 1}, {0, 2}, basic(1));
  EXPECT(plan_side(big, 0x1000, 1, 0, &s, &err) && plan_side(basic(1), (uint64_t)1 << 40, ((int64_t)1 << 32) + 2, 0, &d, &err));
  EXPECT(plan_indexed_seg(s, s.irr->tab.data(), d, nullptr, &sg, &err) == kTypeErrUnsupported && err.find("2^32") != std::string::npos);
}

static void test_overlap() {
  const TypeForm I = basic(5);
  // two interleaved irregular layouts of one buffer that share no byte; the second shifted by one shares some
  const TypeForm even = indexed({1, 2, 1}, {8, 0, 4}, I), odd = indexed({1, 1, 2}, {3, 9, 5}, I);
  SideBytes x, y, z, snd;
  std::string err;
  int a = -1, b = -1;
  EXPECT(plan_side(even, 0x4000, 1, 0, &x, &err) && plan_side(odd, 0x4000, 1, 0, &y, &err) && plan_side(odd, 0x4000, 1, 1, &z, &err));
  EXPECT(strided_overlap({}, std::vector<SideBytes>{x, y}, &a, &b) == kNoOverlap);
  EXPECT(strided_overlap({}, std::vector<SideBytes>{x, z}, &a, &b) == kRecvOverlap && a + b == 1);
  EXPECT(plan_side(I, 0x4000, 1, 7, &snd, &err));  // element 7 lies in no block of x or y; element 8 in x
  EXPECT(strided_overlap(std::vector<SideBytes>{snd}, std::vector<SideBytes>{x, y}, &a, &b) == kNoOverlap);
  EXPECT(plan_side(I, 0x4000, 1, 8, &snd, &err));
  EXPECT(strided_overlap(std::vector<SideBytes>{snd}, std::vector<SideBytes>{x, y}, &a, &b) == kSendRecvOverlap && b == 0);
  // items of one layout step by the extent: 3 items of `even` (extent 9) do not meet themselves
  EXPECT(plan_side(even, 0x4000, 3, 0, &x, &err));
  EXPECT(strided_overlap({}, std::vector<SideBytes>{x}, &a, &b) == kNoOverlap);
  // the span is the true lowest and highest byte: a type with lb = 4 at displacement 0 clears [0, 16)
  const TypeForm hi = indexed({2, 1}, {9, 4}, I);
  EXPECT(plan_side(hi, 0x4000, 2, 0, &x, &err) && plan_side(I, 0x4000, 4, 0, &y, &err));
  uint64_t lo, up;
  x.span(&lo, &up);
  EXPECT(lo == 0x4000 + 16 && up == 0x4000 + (7 + 11) * 4);
  EXPECT(spans_disjoint({}, std::vector<SideBytes>{x, y}));
  // beyond 65,536 blocks where spans meet: unchecked; disjoint spans are settled at any size
  V bl((size_t)kOverlapMaxBlocks, 1), d((size_t)kOverlapMaxBlocks);
  for (size_t i = 0; i < d.size(); i++) d[i] = 3 * (int64_t)i + (i & 1);
  const TypeForm big = indexed(bl, d, basic(1));
  EXPECT(big.irr && plan_side(big, 0x100000, 1, 0, &x, &err) && plan_side(big, 0x100000, 1, 1, &y, &err));
  EXPECT(strided_overlap({}, std::vector<SideBytes>{x, y}, &a, &b) == kOverlapUnchecked);
  EXPECT(plan_side(big, 0x100000 + 3 * kOverlapMaxBlocks, 1, 0, &y, &err));
  EXPECT(strided_overlap({}, std::vector<SideBytes>{x, y}, &a, &b) == kNoOverlap);
}

int main() {
  test_forms();
  test_addresses();
  test_tables_and_granule();
  test_overlap();
  if (failures) {
    printf("indexed_plan_test: %d failures\n", failures);
    return 1;
  }
  printf("indexed_plan_test: ok\n");
  return 0;
}
