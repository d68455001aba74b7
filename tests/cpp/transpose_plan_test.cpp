// transpose_plan_test.cpp — the eligibility test and tile geometry of k_transpose
// (mpjexpress_amd/csrc/mpjx_transpose_plan.hpp) and the planner's handling of types with explicit bounds, on the
// CPU. A stand-alone program: plain g++, no HIP, so it also runs under -fsanitize=address,undefined
// (tests/test_transpose_plan.py).
//   - for each granule (1, 2, 4, 8, 16 B), R and C in {2, T-1, T, T+1, 2T+1} with T the tile side, and both
//     directions: every slot of every tile on both walks, through the functions the kernel calls. Every (r, c)
//     is covered exactly once per walk, every address equals SideBytes::at() of the packed granule, both walks
//     of a slot meet at one LDS offset inside the tile's LDS and no two slots share one, neighbouring lanes
//     touch neighbouring granules on both global sides, and no predicated-off slot is in range
//   - eligibility: the near misses (two granules per block, eb != bb, both sides strided, one row, one item)
//   - launch tables split at kTransposeMax segments and hold the sum of the tiles
//   - plan_side / span() / overlap for interleaved items, an UB below the blocks' end and extent 0
#include <stdio.h>
#include <stdlib.h>

#include <map>
#include <set>

#include "../../mpjexpress_amd/csrc/mpjx_indexed_plan.hpp"
#include "../../mpjexpress_amd/csrc/mpjx_transpose_plan.hpp"

using namespace mpjx;

static int failures = 0;
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
      failures++;                                                       \
    }                                                                   \
  } while (0)

static TypeForm basic(int code) {
  TypeForm f;
  EXPECT(basic_form(code, &f));
  return f;
}

// Vector(R, 1, ld, old) resized to the extent of one `old`: a column of a row-major matrix
static TypeForm column(int64_t R, int64_t ld, int code) {
  const TypeForm old = basic(code);
  TypeForm v, out;
  std::string err;
  EXPECT(vector_any_form(R, 1, ld, old, &v, &err) == kTypeOk);
  const int64_t bl[2] = {1, 1}, disp[2] = {0, old.size()};
  EXPECT(struct_form(2, bl, disp, {v, basic(kCodeUB)}, &out, &err) == kTypeOk);
  return out;
}

static SideBytes side(const TypeForm& f, uint64_t buf, int64_t count, int64_t disp = 0) {
  SideBytes x;
  std::string err;
  EXPECT(plan_side(f, buf, count, disp, &x, &err));
  return x;
}

static void walk(int code, uint32_t glog, int64_t R, int64_t C, bool gather) {
  const TypeForm old = basic(code);
  const int64_t ld = C + 3;  // the panel sits inside a wider matrix
  const TypeForm col = column(R, ld, code);
  EXPECT(!col.irr && col.nblocks == R && col.extent() == old.size() && col.ub_set && !col.lb_set);
  const uint64_t xbuf = 0x7000000000ull + 16 * 5, ybuf = 0x7100000000ull;
  const SideBytes X = side(col, xbuf, C, 2 * old.size());
  TypeForm run;
  std::string err;
  EXPECT(contiguous_of(R * C, old, &run, &err) == kTypeOk);
  const SideBytes Y = side(run, ybuf, 1);
  EXPECT(X.bb == (1 << glog) && X.eb == X.bb && X.nb == R && X.items == C && Y.contiguous());
  TransposeSeg t;
  const bool ok = gather ? plan_transpose_seg(X, Y, &t) : plan_transpose_seg(Y, X, &t);
  EXPECT(ok);
  if (!ok) return;
  EXPECT(t.glog == glog && t.R == (uint32_t)R && t.C == (uint32_t)C && (t.gather != 0) == gather);
  const uint32_t T = tr_tile_side(glog), g = 1u << glog;
  const int64_t tiles = tr_tiles(t);
  EXPECT(tiles == ((R + T - 1) / T) * ((C + T - 1) / T));
  EXPECT(T * tr_pitch(glog) <= kTrLdsBytes && T * T % kTrLanes == 0);
  for (int along_x = 0; along_x < 2; along_x++) {
    std::set<std::pair<uint32_t, uint32_t>> seen;
    for (int64_t x = 0; x < tiles; x++) {
      std::map<uint32_t, uint32_t> lds;  // offset -> slot, within one tile
      uint64_t prev = 0;
      bool prev_on = false;
      for (uint32_t i = 0; i < T * T; i++) {
        const TrSlot s = tr_slot(t, (uint32_t)x, i, along_x != 0);
        EXPECT(s.a < T && s.b < T);
        const bool in = s.r < t.R && s.c < t.C;
        EXPECT(s.on == in);  // no predicated-off slot is in range, no in-range slot is off
        if (!s.on) {
          prev_on = false;
          continue;
        }
        EXPECT(seen.insert({s.r, s.c}).second);
        const uint64_t q = (uint64_t)s.c * R + s.r;
        const uint64_t ax = tr_addr_x(t, s.r, s.c), ay = tr_addr_y(t, s.r, s.c);
        EXPECT(ax == X.at((int64_t)q * g) && ay == Y.at((int64_t)q * g));
        // the walk's own side is read or written with consecutive lanes on consecutive granules
        const uint64_t mine = along_x ? ax : ay;
        if (prev_on && i % kTrLanes != 0 && i % T != 0) EXPECT(mine == prev + g);
        prev = mine;
        prev_on = true;
        const uint32_t off = tr_lds(t, s);
        EXPECT(off % g == 0 && off + g <= kTrLdsBytes);
        EXPECT(lds.emplace(off, i).second);
        // the other walk finds the same granule at the same offset
        const uint32_t j = along_x ? s.b * T + s.a : s.a * T + s.b;
        const TrSlot o = tr_slot(t, (uint32_t)x, j, along_x == 0);
        EXPECT(o.on && o.r == s.r && o.c == s.c && tr_lds(t, o) == off);
      }
      // granule offsets do not overlap either
      uint32_t end = 0;
      for (const auto& e : lds) {
        EXPECT(e.first >= end);
        end = e.first + g;
      }
    }
    EXPECT((int64_t)seen.size() == R * C);
  }
}

static void test_geometry() {
  const int codes[5] = {1, 3, 5, 8, 0x108};  // BYTE SHORT INT DOUBLE DOUBLE2: granules of 1, 2, 4, 8, 16 B
  for (uint32_t glog = 0; glog < 5; glog++) {
    const int64_t T = tr_tile_side(glog);
    EXPECT(T == (glog <= 2 ? 64 : 32));
    const int64_t dims[5] = {2, T - 1, T, T + 1, 2 * T + 1};
    for (int64_t R : dims)
      for (int64_t C : dims)
        for (int gather = 0; gather < 2; gather++) walk(codes[glog], glog, R, C, gather != 0);
  }
}

static void test_pitch() {
  // the transposed reads are `pitch` bytes apart: 17, 33, 65, 66 and 132 dwords
  const uint32_t want[5] = {68, 132, 260, 264, 528};
  for (uint32_t glog = 0; glog < 5; glog++) EXPECT(tr_pitch(glog) == want[glog]);
  // 4-byte banks, 32 of them per 32 lanes (1, 2, 4 B), 64 per 32 lanes (8 B), 64 per 16 lanes (16 B): no two
  // lanes of a group on one bank
  for (uint32_t glog = 0; glog < 5; glog++) {
    const uint32_t lanes = glog == 4 ? 16 : 32, banks = glog >= 3 ? 64 : 32, dw = glog >= 2 ? (1u << glog) / 4 : 1;
    std::set<uint32_t> used;
    for (uint32_t l = 0; l < lanes; l++)
      for (uint32_t w = 0; w < dw; w++) EXPECT(used.insert((l * tr_pitch(glog) / 4 + w) % banks).second);
  }
}

static void test_eligibility() {
  const uint64_t xb = 0x7000000000ull, yb = 0x7100000000ull;
  TransposeSeg t;
  TypeForm run;
  std::string err;
  const TypeForm I = basic(5);
  EXPECT(contiguous_of(40, I, &run, &err) == kTypeOk);
  const SideBytes Y = side(run, yb, 1);
  // the column: eligible in both directions, never with itself on both sides
  const SideBytes X = side(column(8, 11, 5), xb, 5);
  EXPECT(plan_transpose_seg(X, Y, &t) && t.gather == 1 && plan_transpose_seg(Y, X, &t) && t.gather == 0);
  EXPECT(!plan_transpose_seg(X, X, &t) && !plan_transpose_seg(Y, Y, &t));
  // a block of two granules (an odd row stride keeps the granule at 4 B)
  TypeForm v2, two;
  EXPECT(vector_any_form(4, 2, 11, I, &v2, &err) == kTypeOk);
  const int64_t bl[2] = {1, 1}, d2[2] = {0, 2};
  EXPECT(struct_form(2, bl, d2, {v2, basic(kCodeUB)}, &two, &err) == kTypeOk);
  const SideBytes X2 = side(two, xb, 5);
  EXPECT(X2.bb == 8 && X2.eb == 8 && strided_granule_log(X2, Y) == 2 && !plan_transpose_seg(X2, Y, &t));
  // eb != bb: columns two elements apart
  TypeForm v1, wide;
  EXPECT(vector_any_form(8, 1, 11, I, &v1, &err) == kTypeOk);
  EXPECT(struct_form(2, bl, d2, {v1, basic(kCodeUB)}, &wide, &err) == kTypeOk);
  const SideBytes XW = side(wide, xb, 5);
  EXPECT(XW.bb == 4 && XW.eb == 8 && !plan_transpose_seg(XW, Y, &t) && !plan_transpose_seg(Y, XW, &t));
  // both sides strided
  const SideBytes XB = side(column(5, 9, 5), yb, 8);
  EXPECT(XB.total() == X.total() && !plan_transpose_seg(X, XB, &t));
  // the plain Vector (one item), one row, an irregular side
  const SideBytes V = side(v1, xb, 1);
  EXPECT(!plan_transpose_seg(V, side(run, yb, 1), &t));
  TypeForm irr;
  const int64_t ib[2] = {2, 1}, id[2] = {9, 4};
  EXPECT(hindexed_form(2, ib, id, I, &irr, &err) == kTypeOk && irr.irr);
  EXPECT(!plan_transpose_seg(side(irr, xb, 2), Y, &t));
  // a misaligned base lowers the granule below the block: not eligible
  const SideBytes XD = side(column(8, 11, 8), xb + 4, 5);
  EXPECT(strided_granule_log(XD, Y) == 2 && !plan_transpose_seg(XD, Y, &t));
}

static void test_tables() {
  std::vector<TransposeSeg> segs;
  TypeForm run;
  std::string err;
  int64_t total = 0;
  for (int i = 0; i < 2 * kTransposeMax + 3; i++) {
    const int64_t R = 2 + i, C = 3 + (i % 5) * 40;
    EXPECT(contiguous_of(R * C, basic(8), &run, &err) == kTypeOk);
    TransposeSeg t;
    EXPECT(plan_transpose_seg(side(column(R, C + 1, 8), 0x7000000000ull, C), side(run, 0x7100000000ull, 1), &t));
    segs.push_back(t);
    total += tr_tiles(t);
  }
  std::vector<TransposeTable> tabs;
  plan_transpose_tables(segs, &tabs);
  EXPECT(tabs.size() == 3 && tabs[0].n == kTransposeMax && tabs[1].n == kTransposeMax && tabs[2].n == 3);
  int64_t sum = 0;
  size_t k = 0;
  for (const TransposeTable& t : tabs) {
    EXPECT(t.tile0[0] == 0);
    for (int c = 0; c < t.n; c++, k++) {
      EXPECT((int64_t)(t.tile0[c + 1] - t.tile0[c]) == tr_tiles(segs[k]) && t.seg[c].R == segs[k].R);
    }
    sum += t.tile0[t.n];
  }
  EXPECT(sum == total && k == segs.size());
  plan_transpose_tables(segs, &tabs, 4);  // the tile limit closes tables too
  for (const TransposeTable& t : tabs) EXPECT(t.n >= 1 && (t.tile0[t.n] <= 4 || t.n == 1));
}

static void test_bounds_in_the_planner() {
  const TypeForm I = basic(5);
  std::string err;
  const uint64_t buf = 0x7000000000ull;
  // interleaved columns: extent 1 element under a span of 7 * 11 + 1
  const TypeForm col = column(8, 11, 5);
  const SideBytes X = side(col, buf, 5, 3);
  uint64_t lo, hi;
  X.span(&lo, &hi);
  EXPECT(lo == buf + 12 && hi == buf + 12 + (4 * 1 + 7 * 11 + 1) * 4);  // the true lowest and highest byte
  EXPECT(!X.items_may_overlap());                                         // columns of a panel: settled cheaply
  int a = -1, b = -1;
  EXPECT(strided_overlap({}, {X}, &a, &b) == kNoOverlap);
  // twelve columns of a matrix eleven wide: column 11 is column 0 one row down, shared but for the ends
  const SideBytes XO = side(col, buf, 12);
  EXPECT(XO.items_may_overlap() && strided_overlap({}, {XO}, &a, &b) == kRecvOverlap);
  EXPECT(strided_overlap({XO}, {}, &a, &b) == kNoOverlap);  // as a send layout it is fine
  // two receive panels side by side in one matrix interleave without sharing; shifted by less they share
  EXPECT(strided_overlap({}, {side(col, buf, 5), side(col, buf, 6, 5)}, &a, &b) == kNoOverlap);
  EXPECT(strided_overlap({}, {side(col, buf, 5), side(col, buf, 6, 4)}, &a, &b) == kRecvOverlap);
  // an UB below the blocks' end, irregular: blocks [0,2) and [5,6), extent 3
  TypeForm low;
  const int64_t bl[3] = {2, 1, 1}, disp[3] = {0, 5, 3};
  EXPECT(struct_form(3, bl, disp, {I, I, basic(kCodeUB)}, &low, &err) == kTypeOk);
  EXPECT(low.irr && low.extent() == 3 && low.ub() == 3 && low.true_ub() == 6 && low.ub_set);
  const SideBytes Lo = side(low, buf, 4);
  Lo.span(&lo, &hi);
  EXPECT(lo == buf && hi == buf + (3 * 3 + 6) * 4 && Lo.eb == 12 && Lo.total() == 4 * 12);
  EXPECT(Lo.items_may_overlap() && strided_overlap({}, {Lo}, &a, &b) == kNoOverlap);  // 0,1,5 | 3,4,8 | 6,7,11 ...
  EXPECT(Lo.at(0) == buf && Lo.at(8) == buf + 20 && Lo.at(12) == buf + 12);
  TypeForm clash;  // blocks [0,2) and [4,5), extent 2: item 2's first block is item 0's second
  const int64_t d2[3] = {0, 4, 2};
  EXPECT(struct_form(3, bl, d2, {I, I, basic(kCodeUB)}, &clash, &err) == kTypeOk);
  EXPECT(strided_overlap({}, {side(clash, buf, 3)}, &a, &b) == kRecvOverlap);
  EXPECT(strided_overlap({}, {side(clash, buf, 2)}, &a, &b) == kNoOverlap);
  // the count limit follows the true end: (count - 1) * extent + true_ub
  SideBytes x;
  const int64_t lim = kMoveMaxBytes / 4;
  EXPECT(plan_side(low, 0, (lim - 6) / 3 + 1, 0, &x, &err));
  EXPECT(!plan_side(low, 0, (lim - 6) / 3 + 2, 0, &x, &err) && err.find("too large") != std::string::npos);
  // extent 0: every item at the same place; the division is guarded, the size still bounds the count
  TypeForm z;
  const int64_t zb[2] = {2, 1}, zd[2] = {3, 3};
  EXPECT(struct_form(2, zb, zd, {I, basic(kCodeUB)}, &z, &err) == kTypeOk);
  EXPECT(z.extent() == 0 && z.lb() == 3 && z.ub() == 3 && z.size() == 2 && z.true_ub() == 5);
  const SideBytes Z = side(z, buf, 4);
  Z.span(&lo, &hi);
  EXPECT(Z.eb == 0 && Z.total() == 32 && lo == buf + 12 && hi == buf + 20);
  EXPECT(Z.at(0) == buf + 12 && Z.at(8) == buf + 12 && Z.at(28) == buf + 16);
  EXPECT(Z.items_may_overlap() && strided_overlap({}, {Z}, &a, &b) == kRecvOverlap);
  EXPECT(strided_overlap({Z}, {side(I, buf + 4096, 8)}, &a, &b) == kNoOverlap);  // sent, it is legal
  EXPECT(strided_overlap({}, {side(z, buf, 1)}, &a, &b) == kNoOverlap);
  EXPECT(!plan_side(z, 0, lim, 0, &x, &err) && plan_side(z, 0, lim / 2, 0, &x, &err));
  // a negative extent and data at a negative displacement are refused; a marker at one is not
  TypeForm bad;
  const int64_t nb[3] = {1, 1, 1}, nd[3] = {0, 9, 3}, md[3] = {-1, 0, 3}, ld[3] = {0, -3, 3};
  EXPECT(struct_form(3, nb, nd, {I, basic(kCodeLB), basic(kCodeUB)}, &bad, &err) == kTypeErrUnsupported);
  EXPECT(err.find("extent -6") != std::string::npos);
  EXPECT(struct_form(3, nb, md, {I, basic(kCodeLB), basic(kCodeUB)}, &bad, &err) == kTypeErrUnsupported);
  EXPECT(struct_form(3, nb, ld, {I, basic(kCodeLB), basic(kCodeUB)}, &bad, &err) == kTypeOk && bad.lb() == -3 &&
         bad.extent() == 6 && bad.true_lb() == 0);
  // a Vector of a padded element is flattened and comes out regular
  TypeForm pad, vp;
  const int64_t pb[2] = {1, 1}, pd[2] = {0, 3};
  EXPECT(struct_form(2, pb, pd, {I, basic(kCodeUB)}, &pad, &err) == kTypeOk && pad.extent() == 3);
  EXPECT(vector_any_form(3, 2, 4, pad, &vp, &err) == kTypeOk);
  // blocks of 2 padded items (elements 0 and 3) every 12: 0 3 | 12 15 | 24 27
  EXPECT(vp.irr && vp.irr->tab.size() == 6 && vp.irr->tab[3].off == 15 * 4);
  EXPECT(vp.size() == 6 && vp.lb() == 0 && vp.ub() == 2 * 12 + 3 + 3 && vp.ub_set);
  TypeForm cp;
  EXPECT(contiguous_any_form(4, pad, &cp, &err) == kTypeOk && !cp.irr && cp.nblocks == 4 && cp.stride == 3 &&
         cp.extent() == 12 && cp.ub() == 12 && cp.true_ub() == 10);
}

int main() {
  test_geometry();
  test_pitch();
  test_eligibility();
  test_tables();
  test_bounds_in_the_planner();
  if (failures) {
    printf("transpose_plan_test: %d failure(s)\n", failures);
    return 1;
  }
  printf("transpose_plan_test: ok\n");
  return 0;
}
