// wire_plan_test.cpp — the launch table and the per-lane arithmetic of k_wire
// (mpjexpress_amd/csrc/mpjx_wire_plan.hpp) on the CPU. A stand-alone program: plain g++, no HIP;
// tests/test_wire_abi.py builds it with -fsanitize=address,undefined.
//   - walks EVERY lane of every block of both directions with the functions the kernel calls (the table search,
//     wire_check_header, wire_lane, wire_lay_addr, wire_slot_word) over real host buffers: all 14 (granule, word)
//     arms x {linear, Vector, Indexed}, 0 / 1 / 1023 / 1024 / 1025 granules, both tile shapes, and for the unpack
//     every short length n that cuts a granule (r = 1 .. words per granule - 1) in the first granule, across a tile
//     boundary and in the last granule
//   - every byte of the image and of the typed buffer, guards included, against an independent byte-wise model:
//     SideBytes::at plus a byte reversal per word. No byte outside [0, 8 + payload) of the image, or outside the
//     first n elements of the layout, may be written
//   - the header checks in their order; table planning at 1, kWireMax and kWireMax + 1 segments
#include <stdio.h>

#include <iostream>

#include "../../mpjexpress_amd/csrc/mpjx_wire_plan.hpp"

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
using Bytes = std::vector<unsigned char>;
constexpr unsigned char kSentinel = 0xA5;
constexpr size_t kGuard = 64;

static unsigned char rnd() {
  static uint32_t s = 12345;
  s = s * 1664525u + 1013904223u;
  return (unsigned char)(s >> 24);
}

// ---- the kernel's walk: block by block, lane by lane ---------------------------------------------------------------

static void move_words(uint64_t dst, uint64_t src, uint32_t words, uint32_t w) {  // load, swap in "registers", store
  for (uint32_t k = 0; k < words; k++) {
    unsigned char reg[8];
    memcpy(reg, (const void*)(uintptr_t)(src + (uint64_t)k * w), w);
    for (uint32_t j = 0; j < w / 2; j++) std::swap(reg[j], reg[w - 1 - j]);
    memcpy((void*)(uintptr_t)(dst + (uint64_t)k * w), reg, w);
  }
}

static void walk(const WireTable& t, int TH, int U) {
  for (uint32_t g = 0; g < t.tile0[t.n]; g++) {
    int c = 0, hi = t.n;
    while (hi - c > 1) {
      const int mid = (c + hi) >> 1;
      if (t.tile0[mid] <= g) c = mid;
      else hi = mid;
    }
    const WireSeg a = t.seg[c];
    const uint32_t x = g - t.tile0[c];
    const uint32_t G = 1u << a.glog, w = 1u << a.wlog;
    int64_t n = 0;
    if (a.unpack) {
      uint64_t hd;
      memcpy(&hd, (const void*)(uintptr_t)a.hdr, 8);
      const int err = wire_check_header(a, hd, &n);
      if (x == 0) {
        const uint64_t sw = wire_slot_word(err, n);
        memcpy((void*)(uintptr_t)a.slot, &sw, 8);
      }
      if (err) continue;
    } else if (x == 0) {
      memcpy((void*)(uintptr_t)a.hdr, &a.header, 8);
    }
    // the kernel's own form of wire_lane: whole granules below `full`, r words of granule `full`
    const uint64_t full = a.unpack ? ((uint64_t)n << a.wlog) >> a.glog : (uint64_t)a.ngran;
    const uint32_t r = a.unpack ? (uint32_t)((((uint64_t)n << a.wlog) & (G - 1u)) >> a.wlog) : 0u;
    EXPECT(full <= a.ngran && (r == 0 || full < a.ngran));
    for (int tid = 0; tid < TH; tid++)
      for (int u = 0; u < U; u++) {
        const uint64_t q = (uint64_t)x * (uint64_t)(TH * U) + (uint64_t)u * (uint64_t)TH + (uint64_t)tid;
        if (a.unpack) {
          const WireLane l = wire_lane(a, n, q);
          EXPECT(l.whole == (q < full) && l.r == (q == full ? r : 0u));
          if (q >= a.ngran) {
            EXPECT(!l.whole && l.r == 0);  // everything a good header announces lies inside the grid
            continue;
          }
          if (l.whole) move_words(wire_lay_addr(a, (uint32_t)q), a.pay + (q << a.glog), G / w, w);
          else if (l.r) move_words(wire_lay_addr(a, (uint32_t)q), a.pay + (q << a.glog), l.r, w);
        } else if (q < a.ngran) {
          move_words(a.pay + (q << a.glog), wire_lay_addr(a, (uint32_t)q), G / w, w);
        }
      }
  }
}

// ---- layouts --------------------------------------------------------------------------------------------------

enum Kind { kLinear = 0, kVector = 1, kIndexed = 2 };
static const int kBaseOf[4] = {1, 3, 5, 8};  // BYTE, SHORT, INT, DOUBLE: words of 1, 2, 4, 8 bytes

// `ngran` granules of 2^glog bytes of base words of 2^wlog bytes, as one item of a type of the kind; *off is the
// byte offset of the buffer position inside a 16-aligned region (it pins a linear layout's granule)
static TypeForm make_form(Kind kind, int glog, int wlog, int64_t ngran, int64_t* count, uint64_t* off) {
  TypeForm B, f;
  std::string err;
  EXPECT(basic_form(kBaseOf[wlog], &B));
  const int64_t b = (int64_t)1 << (glog - wlog);  // elements per granule
  *count = 1;
  *off = 0;
  if (ngran == 0) {
    *count = 0;
    return B;
  }
  if (kind == kLinear) {
    *count = ngran * b;
    *off = glog < 4 ? (uint64_t)1 << glog : 0;
    return B;
  }
  if (kind == kVector) {
    EXPECT(vector_form(ngran, b, 3 * b, B, &f, &err) == kTypeOk);
    return f;
  }
  V bl, ds;
  for (int64_t i = 0; i < ngran; i++) {
    bl.push_back(b);
    ds.push_back(b * (3 * i + (i & 1)));
  }
  EXPECT(hindexed_form((int64_t)bl.size(), bl.data(), ds.data(), B, &f, &err) == kTypeOk);
  return f;
}

struct Side {
  TypeForm f;
  SideBytes lay;
  std::vector<uint64_t> store;  // 16-aligned backing
  unsigned char* region = nullptr;
  size_t region_bytes = 0;
  unsigned char* buf = nullptr;  // the buffer position
};

static void make_side(Kind kind, int glog, int wlog, int64_t ngran, Side* s) {
  int64_t count = 0;
  uint64_t off = 0;
  s->f = make_form(kind, glog, wlog, ngran, &count, &off);
  const int64_t span = count > 0 ? ((count - 1) * s->f.extent() + s->f.true_ub()) * s->f.bsz : 0;
  s->region_bytes = kGuard + (size_t)off + (size_t)span + kGuard;
  s->store.assign(s->region_bytes / 8 + 4, 0);
  s->region = (unsigned char*)(((uintptr_t)s->store.data() + 15) & ~(uintptr_t)15);
  s->buf = s->region + kGuard + off;
  std::string err;
  EXPECT(plan_side(s->f, (uint64_t)(uintptr_t)s->buf, count, 0, &s->lay, &err));
  EXPECT(s->lay.total() == (ngran << glog));
}

struct Image {
  std::vector<uint64_t> store;
  unsigned char* region = nullptr;  // 16-aligned; the image starts kGuard + 8 bytes in: its payload is 16-aligned
  size_t region_bytes = 0;
  unsigned char* img = nullptr;
};

static void make_image(int64_t bytes, Image* im) {
  im->region_bytes = kGuard + 8 + (size_t)bytes + kGuard;
  im->store.assign(im->region_bytes / 8 + 4, 0);
  im->region = (unsigned char*)(((uintptr_t)im->store.data() + 15) & ~(uintptr_t)15);
  im->img = im->region + kGuard + 8;
}

static const IdxEnt* tab_of(const SideBytes& lay) { return lay.irr ? lay.irr->tab.data() : nullptr; }

static void run(const WireSeg& sg, bool nt) {
  std::vector<WireTable> tabs;
  plan_wire_tables({sg}, nt ? kStridedTileNT : kStridedTile, &tabs);
  EXPECT(tabs.size() == 1 && tabs[0].n == 1 && tabs[0].tile0[1] >= 1);
  walk(tabs[0], nt ? 512 : 256, nt ? 1 : 4);
}

// ---- pack -----------------------------------------------------------------------------------------------------

static void pack_case(Kind kind, int glog, int wlog, int64_t ngran, bool nt) {
  Side s;
  make_side(kind, glog, wlog, ngran, &s);
  const int64_t payload = s.lay.total(), w = (int64_t)1 << wlog;
  Image im;
  make_image(8 + payload, &im);
  for (size_t i = 0; i < s.region_bytes; i++) s.region[i] = rnd();
  memset(im.region, kSentinel, im.region_bytes);
  const Bytes src(s.region, s.region + s.region_bytes);
  WireSeg sg;
  plan_wire_pack(s.lay, tab_of(s.lay), (uint64_t)(uintptr_t)im.img, s.f.base, s.f.bsz, &sg);
  EXPECT((int)sg.glog == (ngran ? glog : wlog) && (int)sg.wlog == wlog && sg.ngran == (uint32_t)ngran && sg.unpack == kWirePack);
  run(sg, nt);
  // the model, byte by byte
  Bytes want(im.region_bytes, kSentinel);
  unsigned char* wi = want.data() + kGuard + 8;
  const uint32_t nw = (uint32_t)(payload / w);
  const unsigned char hdr[8] = {(unsigned char)(s.f.base - 1), 0, 0, 0, (unsigned char)(nw >> 24), (unsigned char)(nw >> 16),
                                (unsigned char)(nw >> 8), (unsigned char)nw};
  memcpy(wi, hdr, 8);
  for (int64_t p = 0; p < payload; p++) {
    const int64_t word = p / w, j = p % w;
    wi[8 + p] = *(const unsigned char*)(uintptr_t)s.lay.at(word * w + (w - 1 - j));
  }
  EXPECT(memcmp(want.data(), im.region, im.region_bytes) == 0);
  EXPECT(memcmp(src.data(), s.region, s.region_bytes) == 0);  // the source is only read
}

// ---- unpack ---------------------------------------------------------------------------------------------------

static void put_header(unsigned char* img, int code, int64_t n) {
  const uint32_t v = (uint32_t)n;
  const unsigned char hdr[8] = {(unsigned char)code, 0, 0, 0, (unsigned char)(v >> 24), (unsigned char)(v >> 16),
                                (unsigned char)(v >> 8), (unsigned char)v};
  memcpy(img, hdr, 8);
}

// n words announced to a layout of `ngran` granules, `sent` image bytes; want_err: the code expected
static void unpack_case(Kind kind, int glog, int wlog, int64_t ngran, int64_t n, int64_t sent, bool nt, int want_err = 0,
                        int code_delta = 0) {
  Side s;
  make_side(kind, glog, wlog, ngran, &s);
  const int64_t w = (int64_t)1 << wlog;
  Image im;
  make_image(sent, &im);
  for (size_t i = 0; i < im.region_bytes; i++) im.region[i] = rnd();
  put_header(im.img, s.f.base - 1 + code_delta, n);
  memset(s.region, kSentinel, s.region_bytes);
  const Bytes src(im.region, im.region + im.region_bytes);
  uint64_t slot = ~(uint64_t)0;
  WireSeg sg;
  plan_wire_unpack(s.lay, tab_of(s.lay), (uint64_t)(uintptr_t)im.img, sent, s.f.base, s.f.bsz, (uint64_t)(uintptr_t)&slot, &sg);
  EXPECT(sg.unpack == kWireUnpack && sg.cap == s.lay.total() / w && sg.sent == sent);
  EXPECT(((int64_t)sg.ngran << sg.glog) >= std::min<int64_t>(s.lay.total(), sent - 8));
  EXPECT(((int64_t)sg.ngran << sg.glog) <= s.lay.total());
  run(sg, nt);
  int32_t got[2];
  memcpy(got, &slot, 8);
  EXPECT(got[0] == want_err && got[1] == (int32_t)n);
  Bytes want(s.region_bytes, kSentinel);
  if (!want_err)
    for (int64_t p = 0; p < n * w; p++) {
      const int64_t word = p / w, j = p % w;
      want[(size_t)(s.lay.at(p) - (uint64_t)(uintptr_t)s.region)] = im.img[8 + word * w + (w - 1 - j)];
    }
  EXPECT(memcmp(want.data(), s.region, s.region_bytes) == 0);
  EXPECT(memcmp(src.data(), im.region, im.region_bytes) == 0);  // the image is only read
}

static void test_matrix() {
  const int64_t grans[] = {0, 1, 1023, 1024, 1025};
  int arms = 0;
  for (int wlog = 0; wlog <= 3; wlog++)
    for (int glog = wlog; glog <= 4; glog++) {
      arms++;
      const int64_t wpg = (int64_t)1 << (glog - wlog);  // words per granule
      for (int kind = 0; kind < 3; kind++)
        for (int64_t ng : grans)
          for (int nt = 0; nt < 2; nt++) {
            if (nt && ng != 1025 && ng != 0) continue;  // the second tile shape at the largest size (three tiles of 512) and at none
            pack_case((Kind)kind, glog, wlog, ng, nt);
            const int64_t cap = ng * wpg, w = (int64_t)1 << wlog;
            unpack_case((Kind)kind, glog, wlog, ng, cap, 8 + cap * w, nt);  // the full layout
            unpack_case((Kind)kind, glog, wlog, ng, 0, 8 + cap * w, nt);    // a header that announces 0
            if (ng == 0) continue;
            unpack_case((Kind)kind, glog, wlog, ng, cap - wpg, 8 + (cap - wpg) * w, nt);  // whole granules, one short
            for (int64_t r = 1; r < wpg; r++)                                              // every cut
              for (int64_t qcut : {(int64_t)0, (int64_t)1023, ng - 1}) {
                if (qcut >= ng) continue;
                const int64_t n = qcut * wpg + r;
                unpack_case((Kind)kind, glog, wlog, ng, n, 8 + n * w, nt);      // the image ends with its section
                if (r == 1) unpack_case((Kind)kind, glog, wlog, ng, n, 8 + cap * w + 24, nt);  // a longer image
              }
          }
    }
  EXPECT(arms == 14);
}

static void test_header_checks() {
  // DOUBLE into 16 granules of 16 B (32 words): the order is type, overrun, count
  const int g = 4, w = 3;
  unpack_case(kVector, g, w, 16, 3, 8 + 32 * 8, false, kWireBadType, 1);
  unpack_case(kVector, g, w, 16, -1, 8 + 32 * 8, false, kWireOverrun);
  unpack_case(kVector, g, w, 16, 5, 8 + 4 * 8, false, kWireOverrun);  // n * w past the bytes sent
  unpack_case(kVector, g, w, 16, 5, 8 + 5 * 8 - 1, false, kWireOverrun);
  unpack_case(kVector, g, w, 16, 33, 8 + 40 * 8, false, kWireBadCount);  // n above the room
  unpack_case(kVector, g, w, 16, 40, 8 + 32 * 8, false, kWireOverrun);   // both: overrun comes first
  unpack_case(kVector, g, w, 16, 40, 8 + 32 * 8, false, kWireBadType, 3);
  unpack_case(kLinear, g, w, 0, 1, 8 + 8, false, kWireBadCount);  // an empty layout takes only 0
  unpack_case(kLinear, g, w, 16, 0x7fffffff, 8 + 32 * 8, false, kWireOverrun);
  // 3 doubles into 16-byte blocks cut a granule; SHORT and BYTE analogues
  unpack_case(kVector, 4, 3, 8, 3, 8 + 24, false);
  unpack_case(kVector, 4, 1, 8, 11, 8 + 22, false);
  unpack_case(kVector, 4, 0, 8, 21, 8 + 21, false);
  EXPECT(wire_header_count(pack_header_word(5, 0x01020304)) == 0x01020304);
  EXPECT(wire_header_count(pack_header_word(5, 0xffffffffll)) == -1);
}

static void test_tables() {
  EXPECT(kWireMax >= 16 && sizeof(WireTable) <= 4096);
  WireSeg one{};
  one.ngran = 2500;
  WireSeg none{};  // header only: still one tile
  for (int n : {1, kWireMax, kWireMax + 1}) {
    std::vector<WireSeg> segs;
    for (int i = 0; i < n; i++) segs.push_back(i % 2 ? none : one);
    std::vector<WireTable> tabs;
    plan_wire_tables(segs, kStridedTile, &tabs);
    EXPECT(tabs.size() == (n > kWireMax ? 2u : 1u));
    int total = 0;
    for (const WireTable& t : tabs) {
      EXPECT(t.n >= 1 && t.n <= kWireMax && t.tile0[0] == 0);
      for (int c = 0; c < t.n; c++) {
        const uint32_t tiles = t.tile0[c + 1] - t.tile0[c];
        EXPECT(tiles == (t.seg[c].ngran ? 3u : 1u));
      }
      total += t.n;
    }
    EXPECT(total == n);
    plan_wire_tables(segs, kStridedTileNT, &tabs);
    EXPECT(tabs[0].tile0[1] == 5u);
  }
  // a table closes at max_tiles too
  std::vector<WireTable> tabs;
  plan_wire_tables({one, one, one}, kStridedTile, &tabs, 6);
  EXPECT(tabs.size() == 2 && tabs[0].n == 2 && tabs[1].n == 1);
}

int main() {
  test_matrix();
  test_header_checks();
  test_tables();
  if (failures) {
    printf("wire_plan_test: %d failure(s)\n", failures);
    return 1;
  }
  printf("wire_plan_test: ok\n");
  return 0;
}
