// pack_plan_test.cpp — the planner of mpjx_pack / mpjx_unpack / mpjx_pack_size
// (mpjexpress_amd/csrc/mpjx_pack_plan.hpp) on the CPU. A stand-alone program: plain g++, no HIP;
// tests/test_pack_abi.py builds it with -fsanitize=address,undefined.
//   - the section arithmetic at positions 0, 5, 8 and 11, the int32 limit of the header's count, the image bound
//   - Pack_size's known values, padding quirk included
//   - the 8 header bytes
//   - the granule: an 8-aligned payload against a 16-aligned one, never below the base word
//   - for EVERY granule of a set of layouts (contiguous, Vector, Indexed with lb > 0, 600 reversed blocks) the
//     kernel's buffer-side address against SideBytes::at, and the payload side linear
// With --cases it plans the cases given on stdin instead and prints each one's cell (run_cases below;
// tests/test_pack_cases.py feeds it tests/pack_cases.py).
#include <stdio.h>

#include <iostream>

#include "../../mpjexpress_amd/csrc/mpjx_pack_plan.hpp"

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
static TypeForm vec(int64_t c, int64_t b, int64_t s, const TypeForm& old) {
  TypeForm f;
  std::string err;
  EXPECT(vector_form(c, b, s, old, &f, &err) == kTypeOk);
  return f;
}
static TypeForm indexed(const V& bl, const V& d, const TypeForm& old, bool h = false) {
  TypeForm f;
  std::string err;
  EXPECT((h ? hindexed_form : indexed_form)((int64_t)bl.size(), bl.data(), d.data(), old, &f, &err) == kTypeOk);
  return f;
}

static bool section(int64_t pos, int64_t count, const TypeForm& f, int64_t image_bytes, PackSection* s,
                    std::string* err = nullptr) {
  std::string e;
  const bool ok = plan_pack_section(pos, count, f.size(), f.bsz, image_bytes, s, &e);
  EXPECT(ok == e.empty());
  if (err) *err = e;
  return ok;
}

static void test_section() {
  const TypeForm B = basic(1), I = basic(5), D = basic(8), F2 = basic(0x107);
  const TypeForm v = vec(3, 2, 5, I);
  PackSection s;
  // position -> header: 0 -> 0, 5 -> 8, 8 -> 8, 11 -> 16
  EXPECT(section(0, 3, B, 64, &s) && s.h == 0 && s.pay == 8 && s.end == 11 && s.words == 3);
  EXPECT(section(5, 3, B, 64, &s) && s.h == 8 && s.pay == 16 && s.end == 19);
  EXPECT(section(8, 1, D, 64, &s) && s.h == 8 && s.pay == 16 && s.end == 24 && s.words == 1);
  EXPECT(section(11, 2, v, 72, &s) && s.h == 16 && s.pay == 24 && s.end == 72 && s.words == 12);
  EXPECT(section(0, 3, F2, 32, &s) && s.words == 6 && s.end == 32);  // a pair is 2 base elements
  // count 0: a header alone
  EXPECT(section(5, 0, D, 16, &s) && s.h == 8 && s.end == 16 && s.words == 0);
  // the image bound is what the section really needs
  std::string err;
  EXPECT(section(11, 2, v, 72, &s) && !section(11, 2, v, 71, &s, &err) && err.find("71") != std::string::npos);
  EXPECT(!section(5, 0, D, 15, &s) && !section(9, 0, D, 16, &s) && !section(17, 0, B, 16, &s));
  EXPECT(section(0, 0, B, 8, &s) && !section(0, 0, B, 7, &s) && !section(0, 1, B, 8, &s) && section(0, 1, B, 9, &s));
  // negatives
  EXPECT(!section(-1, 1, I, 64, &s, &err) && err.find("position -1") != std::string::npos);
  EXPECT(!section(0, -2, I, 64, &s, &err) && err.find("count -2") != std::string::npos);
  EXPECT(!section(0, 1, I, -64, &s));
  // the header's count is a Java int: count * Size() <= 2^31 - 1
  const int64_t big = (int64_t)1 << 40;
  EXPECT(section(0, 0x7fffffff, B, big, &s) && s.words == 0x7fffffff && s.end == 8 + (int64_t)0x7fffffff);
  EXPECT(!section(0, (int64_t)0x7fffffff + 1, B, big, &s, &err) && err.find("int32") != std::string::npos);
  EXPECT(section(0, 0x7fffffff / 6, v, big, &s) && !section(0, 0x7fffffff / 6 + 1, v, big, &s));  // 6 ints per item
  EXPECT(!section(0, (int64_t)1 << 62, D, big, &s) && !section(0, INT64_MAX, F2, big, &s));
  // positions near the top of the range neither overflow nor pass
  EXPECT(!section(INT64_MAX, 0, B, INT64_MAX, &s) && !section(INT64_MAX - 8, 1, B, INT64_MAX, &s));
}

static void test_pack_size() {
  auto ps = [](int64_t count, const TypeForm& f) { return pack_size_bytes(count, f.size() * f.bsz); };
  EXPECT(ps(1, basic(1)) == 10);  // t = 9, + 9 % 8
  EXPECT(ps(3, basic(1)) == 14);  // t = 11, + 3
  EXPECT(ps(1, basic(3)) == 12);  // t = 10, + 2
  EXPECT(ps(1, basic(5)) == 16);  // t = 12, + 4
  EXPECT(ps(1, basic(8)) == 16);
  EXPECT(ps(2, vec(3, 2, 5, basic(5))) == 56);
  EXPECT(ps(0, basic(8)) == 8);
  EXPECT(ps(7, basic(1)) == 22);  // t = 15, + 7: the quirk at its widest
}

static void test_header() {
  auto bytes = [](uint64_t w, std::initializer_list<int> want) {
    unsigned char b[8];
    memcpy(b, &w, 8);
    int i = 0;
    bool ok = true;
    for (int x : want) ok = ok && b[i++] == x;
    return ok;
  };
  EXPECT(bytes(pack_header_word(5, 12), {4, 0, 0, 0, 0, 0, 0, 12}));
  EXPECT(bytes(pack_header_word(8, 0x01020304), {7, 0, 0, 0, 1, 2, 3, 4}));
  EXPECT(bytes(pack_header_word(1, 0x7fffffff), {0, 0, 0, 0, 0x7f, 0xff, 0xff, 0xff}));
  EXPECT(bytes(pack_header_word(3, 0), {2, 0, 0, 0, 0, 0, 0, 0}));
}

// One descriptor: `count` items of f at buffer address buf, the section at `pos` of the image at `image`
static PackSeg seg(const TypeForm& f, uint64_t buf, int64_t count, uint64_t image, int64_t pos, SideBytes* lay_out = nullptr) {
  PackSection s;
  EXPECT(section(pos, count, f, (int64_t)1 << 40, &s));
  SideBytes lay;
  std::string err;
  EXPECT(plan_side(f, buf, count, 0, &lay, &err));
  PackSeg sg;
  // the host table stands for the device one: indexed_addr reads it where it lies
  plan_pack_seg(lay, lay.irr ? lay.irr->tab.data() : nullptr, image, (int64_t)1 << 40, s, f.base, f.bsz, nullptr, &sg);
  EXPECT(sg.pay == image + (uint64_t)s.pay && sg.hdr == image + (uint64_t)s.h && sg.words == s.words);
  EXPECT(sg.room == ((int64_t)1 << 40) - s.pay && sg.code == f.base - 1 && (1 << sg.wlog) == f.bsz);
  EXPECT(sg.glog >= sg.wlog && sg.glog <= 4);
  EXPECT((int64_t)sg.ngran << sg.glog == s.words * f.bsz);
  if (lay_out) *lay_out = lay;
  return sg;
}

static void test_granule() {
  const TypeForm B = basic(1), S = basic(3), I = basic(5), D = basic(8), D2 = basic(0x108);
  const uint64_t buf = 0x10000, img = 0x40000;
  // the payload of a section at position 0 is only 8-aligned (image + 8); at position 8 it is 16-aligned
  EXPECT(seg(D, buf, 64, img, 0).glog == 3 && seg(D, buf, 64, img, 8).glog == 4);
  EXPECT(seg(B, buf, 64, img, 0).glog == 3 && seg(B, buf, 64, img, 8).glog == 4 && seg(B, buf, 64, img, 5).glog == 4);
  EXPECT(seg(D2, buf, 4, img, 8).glog == 4 && seg(D2, buf, 4, img, 8).wlog == 3);
  // the buffer side caps it: an odd element address, an odd length
  EXPECT(seg(B, buf + 1, 64, img, 8).glog == 0 && seg(S, buf + 2, 64, img, 8).glog == 1);
  EXPECT(seg(I, buf + 4, 64, img, 8).glog == 2 && seg(D, buf + 8, 64, img, 8).glog == 3);
  EXPECT(seg(B, buf, 3, img, 8).glog == 0 && seg(I, buf, 3, img, 8).glog == 2);
  // never below the base word, whatever the layout: odd block lengths of SHORT give granule 2
  EXPECT(seg(vec(3, 1, 3, S), buf, 5, img, 0).glog == 1 && seg(vec(3, 3, 5, D), buf, 2, img, 0).glog == 3);
  EXPECT(seg(vec(4, 2, 6, I), buf, 2, img, 8).glog == 3 && seg(vec(4, 4, 8, I), buf, 2, img, 8).glog == 4);
  // count 0: nothing to move, the word size still set
  const PackSeg z = seg(D, buf, 0, img, 5);
  EXPECT(z.ngran == 0 && z.wlog == 3 && z.glog == 3 && z.header == pack_header_word(8, 0));
  // contiguous layouts are linear on both sides
  EXPECT(seg(D, buf, 9, img, 0).lin == 1 && seg(vec(1, 5, 9, D), buf, 3, img, 0).lin == 1);
  EXPECT(seg(vec(3, 2, 5, I), buf, 2, img, 0).lin == 0);
}

// Every granule, tile by tile as the kernel's lanes go
static void walk(const TypeForm& f, uint64_t buf, int64_t count, int64_t pos) {
  SideBytes lay;
  const uint64_t img = 0x4000000;
  const PackSeg sg = seg(f, buf, count, img, pos, &lay);
  const int64_t gran = 1024;
  int64_t seen = 0;
  for (int64_t x = 0; x < strided_tiles(sg.ngran, gran); x++)
    for (int64_t t = 0; t < gran; t++) {
      const uint64_t q = (uint64_t)x * gran + t;
      if (q >= sg.ngran) continue;
      EXPECT(pack_lay_addr(sg, (uint32_t)q) == lay.at((int64_t)(q << sg.glog)));
      seen++;
    }
  EXPECT(seen == sg.ngran);
  // every byte of a granule lies in one block: its last byte is where `at` puts it
  const int64_t g = (int64_t)1 << sg.glog;
  for (uint32_t q = 0; q < sg.ngran; q++)
    EXPECT(pack_lay_addr(sg, q) + (uint64_t)(g - 1) == lay.at((int64_t)q * g + g - 1));
}

static void test_addresses() {
  const TypeForm S = basic(3), I = basic(5), D = basic(8), F2 = basic(0x107);
  for (int64_t pos : {0, 5, 8}) {
    for (int64_t count : {1, 3, 1025}) walk(D, 0x10000, count, pos);
    walk(vec(3, 2, 5, I), 0x10004, 2, pos);
    walk(vec(3, 2, 5, F2), 0x10008, 2, pos);
    walk(vec(3, 1, 3, S), 0x10002, 7, pos);
    walk(indexed({3, 1, 2}, {8, 0, 4}, D), 0x10000, 3, pos);
    walk(indexed({2, 2, 2}, {1, 11, 5}, I, true), 0x10000, 3, pos);  // lb = 1, not subtracted
  }
  V bl(600, 1), d(600);
  for (int i = 0; i < 600; i++) d[(size_t)i] = 2 * (599 - i);
  const TypeForm rev = indexed(bl, d, I);
  EXPECT(rev.irr && rev.irr->tab.size() == 600);
  walk(rev, 0x10000, 2, 0);
}

// --cases: one case of tests/pack_cases.py per line of stdin,
//   <base code> B 0 | V 3 <count> <blocklength> <stride> | I 2n <n blocklengths> <n displacements>
//   <count> <buffer offset in base elements> <position>
// planned over a 16-byte aligned buffer and image. Prints per case
//   glog wlog lin tab nb ngran lo hi
// (tab: the layout has a block table; nb: its blocks; lo, hi: the bytes of the buffer the layout touches, from the
// buffer's start). A case of up to 4096 granules has every granule's address walked as above.
static int run_cases() {
  const uint64_t buf = 0x10000000, img = 0x40000000;
  long long code, k, v;
  char ctor;
  int n = 0;
  while (std::cin >> code >> ctor >> k) {
    V a;
    for (long long i = 0; i < k + 3 && (std::cin >> v); i++) a.push_back(v);
    if ((long long)a.size() != k + 3 || k < 0 || (ctor == 'B' && k != 0) || (ctor == 'V' && k != 3) ||
        (ctor == 'I' && (k % 2 || k == 0)) || (ctor != 'B' && ctor != 'V' && ctor != 'I')) {
      printf("case %d: malformed\n", n);
      return 2;
    }
    const TypeForm b = basic((int)code);
    const size_t h = (size_t)k / 2;
    const TypeForm f = ctor == 'B'   ? b
                       : ctor == 'V' ? vec(a[0], a[1], a[2], b)
                                     : indexed(V(a.begin(), a.begin() + (long)h), V(a.begin() + (long)h, a.begin() + (long)k), b);
    const int64_t count = a[(size_t)k], off = a[(size_t)k + 1], pos = a[(size_t)k + 2];
    const uint64_t at = buf + (uint64_t)(off * f.bsz);
    SideBytes lay;
    const PackSeg sg = seg(f, at, count, img, pos, &lay);
    uint64_t lo, hi;
    lay.span(&lo, &hi);
    if (sg.ngran <= 4096) walk(f, at, count, pos);
    printf("%u %u %u %d %u %u %lld %lld\n", sg.glog, sg.wlog, sg.lin, sg.lay.tab ? 1 : 0, sg.lay.r.nb.d, sg.ngran,
           (long long)(lo - buf), (long long)(hi - buf));
    n++;
  }
  if (failures) {
    printf("pack_plan_test: %d failure(s)\n", failures);
    return 1;
  }
  printf("pack_plan_test: ok (%d cases)\n", n);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && std::string(argv[1]) == "--cases") return run_cases();
  test_section();
  test_pack_size();
  test_header();
  test_granule();
  test_addresses();
  if (failures) {
    printf("pack_plan_test: %d failure(s)\n", failures);
    return 1;
  }
  printf("pack_plan_test: ok\n");
  return 0;
}
