// reduce_dt_plan_test.cpp — the host-side planner of the reductions on derived datatypes on the CPU: plain g++,
// no HIP (tests/test_reduce_dt_abi.py builds it under -fsanitize=address,undefined). It walks the functions
// k_pway_dt calls (mpjexpress_amd/csrc/mpjx_reduce_dt_plan.hpp) against a block list expanded here:
//   - the byte offset of EVERY granule of a layout, in the element form and in the 16-B form;
//   - the choice between the two over the layout and the P send + Q receive pointers, and over the layouts and
//     pointer residues of the GPU instantiation matrix;
//   - Reduce_scatter's ranges and the rebasing of the receiving rank's pointer;
//   - same_form on types built twice, and on types that differ.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../mpjexpress_amd/csrc/mpjx_reduce_dt_plan.hpp"

using namespace mpjx;

static int fails = 0;
#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
      fails++;                                                    \
    }                                                             \
  } while (0)

static TypeForm basic(int code) {
  TypeForm f;
  CHECK(basic_form(code, &f));
  return f;
}
static TypeForm vec(int64_t c, int64_t b, int64_t s, const TypeForm& old) {
  TypeForm f;
  std::string err;
  CHECK(vector_form(c, b, s, old, &f, &err) == kTypeOk);
  f.pair = old.pair;
  return f;
}
static TypeForm indexed(std::vector<int64_t> bl, std::vector<int64_t> d, const TypeForm& old, bool h = false) {
  TypeForm f;
  std::string err;
  const int rc = h ? hindexed_form((int64_t)bl.size(), bl.data(), d.data(), old, &f, &err)
                   : indexed_form((int64_t)bl.size(), bl.data(), d.data(), old, &f, &err);
  CHECK(rc == kTypeOk);
  f.pair = old.pair;
  return f;
}

// The byte offsets of the packed bytes of `items` items of f from the buffer position, from its block list
static std::vector<uint64_t> expand(const TypeForm& f, int64_t items) {
  std::vector<uint64_t> at;
  for (int64_t k = 0; k < items; k++)
    for (int64_t b = 0; b < form_nblocks(f); b++) {
      int64_t off, len;
      form_block(f, b, &off, &len);
      for (int64_t i = 0; i < len * f.bsz; i++) at.push_back((uint64_t)((k * f.extent() + off) * f.bsz + i));
    }
  return at;
}

// Every granule of `items` items of f at granule 2^glog: offset == the expanded list's, and the granule's bytes
// are consecutive there (it does not straddle a block)
static void walk(const TypeForm& f, int64_t items, uint32_t glog, const char* what) {
  SideBytes lay;
  std::string err;
  CHECK(reduce_dt_layout(f, items, &lay, &err));
  const std::vector<uint64_t> at = expand(f, items);
  CHECK((int64_t)at.size() == lay.total());
  IndexedSide side;
  int64_t ngran = 0;
  CHECK(plan_reduce_dt(lay, glog, lay.irr ? lay.irr->tab.data() : nullptr, &side, &ngran, &err) == kTypeOk);
  CHECK(ngran == (int64_t)(at.size() >> glog) && (at.size() & ((1u << glog) - 1)) == 0);
  int bad = 0;
  for (int64_t q = 0; q < ngran; q++) {
    const uint64_t o = reduce_dt_offset(side, (uint32_t)q, glog);
    for (uint32_t i = 0; i < (1u << glog); i++) bad += o + i != at[(size_t)((q << glog) + i)];
  }
  if (bad) printf("  %s x%lld glog %u: %d bytes off\n", what, (long long)items, glog, bad);
  CHECK(bad == 0);
}

static void offsets() {
  const TypeForm INT = basic(5), DBL = basic(8), BYTE = basic(1), D2 = basic(0x108);
  for (int64_t n : {1, 3, 7}) {
    walk(vec(6, 2, 5, INT), n, 2, "Vector(6,2,5) INT");
    walk(vec(9, 4, 10, DBL), n, 3, "Vector(9,4,10) DOUBLE elements");
    walk(vec(9, 4, 10, DBL), n, 4, "Vector(9,4,10) DOUBLE 16 B");
    walk(vec(33, 1, 17, DBL), n, 3, "a column");
    walk(vec(5, 3, 7, BYTE), n, 0, "Vector(5,3,7) BYTE");
    walk(vec(5, 16, 48, BYTE), n, 4, "Vector(5,16,48) BYTE 16 B");
    walk(vec(3, 2, 4, D2), n, 4, "Vector(3,2,4) DOUBLE2");
    walk(vec(4, 3, 3, INT), n, 2, "a Vector that is contiguous");
    walk(indexed({2, 1}, {9, 4}, INT), n, 2, "Indexed([2,1],[9,4])");
    walk(indexed({3, 1, 2}, {8, 0, 4}, INT), n, 2, "Indexed back and forth");
    walk(indexed({2, 2, 2}, {1, 11, 5}, INT, true), n, 2, "Hindexed, lb = 1");
    walk(indexed({2}, {3}, INT), n, 2, "one block at lb = 3");
    walk(indexed({4, 8}, {12, 0}, DBL), n, 4, "Indexed DOUBLE 16 B");
    walk(indexed({4, 8}, {12, 0}, DBL), n, 3, "Indexed DOUBLE elements");
    walk(indexed({1, 2}, {4, 0}, D2), n, 4, "Indexed DOUBLE2");
  }
  walk(vec(409, 4, 6, INT), 1, 2, "three tiles and a bit");
  // 2^32 granules or more
  SideBytes lay;
  std::string err;
  CHECK(reduce_dt_layout(vec(2, (int64_t)1 << 31, (int64_t)1 << 32, BYTE), 1, &lay, &err));
  IndexedSide side;
  int64_t ngran;
  CHECK(plan_reduce_dt(lay, 0, nullptr, &side, &ngran, &err) == kTypeErrUnsupported);
  CHECK(err.find("2^32") != std::string::npos);
  CHECK(plan_reduce_dt(lay, 4, nullptr, &side, &ngran, &err) == kTypeOk && ngran == (int64_t)1 << 28);
}

static void granule() {
  const TypeForm DBL = basic(8), INT = basic(5), D2 = basic(0x108), BYTE = basic(1);
  SideBytes lay;
  std::string err;
  CHECK(reduce_dt_layout(vec(9, 4, 10, DBL), 2, &lay, &err));  // 32-B blocks, 80-B stride, 672-B extent
  const uint64_t ok[6] = {0x1000, 0x2010, 0x3000, 0x7f00, 0x100, 0x20};
  CHECK(reduce_dt_granule_log(lay, 8, ok, 6) == 4);
  for (int i = 0; i < 6; i++) {  // any one of the P + Q pointers 8 B further: the element form
    uint64_t p[6];
    for (int j = 0; j < 6; j++) p[j] = ok[j] + (j == i ? 8 : 0);
    CHECK(reduce_dt_granule_log(lay, 8, p, 6) == 3);
  }
  CHECK(reduce_dt_layout(vec(9, 3, 10, DBL), 2, &lay, &err));  // 24-B blocks
  CHECK(reduce_dt_granule_log(lay, 8, ok, 6) == 3);
  CHECK(reduce_dt_layout(vec(9, 4, 9, DBL), 2, &lay, &err));  // 72-B stride
  CHECK(reduce_dt_granule_log(lay, 8, ok, 6) == 3);
  CHECK(reduce_dt_layout(vec(6, 2, 5, INT), 3, &lay, &err));
  CHECK(reduce_dt_granule_log(lay, 4, ok, 6) == 2);
  CHECK(reduce_dt_layout(vec(5, 3, 7, BYTE), 3, &lay, &err));
  CHECK(reduce_dt_granule_log(lay, 1, ok, 6) == 0);
  CHECK(reduce_dt_layout(vec(3, 2, 4, D2), 2, &lay, &err));  // pairs of 16 B: the element IS 16 B
  CHECK(reduce_dt_elem_bytes(vec(3, 2, 4, D2)) == 16 && reduce_dt_elem_bytes(vec(3, 2, 4, DBL)) == 8);
  uint64_t odd[2] = {0x1008, 0x2000};
  CHECK(reduce_dt_granule_log(lay, 16, odd, 2) == 4);
  // an irregular type: every block offset and length and the extent count (IrrLayout::amask)
  CHECK(reduce_dt_layout(indexed({4, 8}, {12, 0}, DBL), 2, &lay, &err));
  CHECK(reduce_dt_granule_log(lay, 8, ok, 6) == 4);
  CHECK(reduce_dt_layout(indexed({4, 8}, {13, 0}, DBL), 2, &lay, &err));  // a block 104 B in
  CHECK(reduce_dt_granule_log(lay, 8, ok, 6) == 3);
  CHECK(reduce_dt_layout(indexed({2}, {3}, INT), 4, &lay, &err));  // one block 12 B in: the offset is in the layout
  CHECK(reduce_dt_granule_log(lay, 4, ok, 6) == 2);
}

// The layouts and pointer residues of tests/test_gpu_reduce_dt_matrix.py (reduce_dt_cases.matrix_spec and
// matrix_widths), which cannot observe the width a call took: Vector(3, 32 B, 48 B) of every type takes the 16-B
// form where all P send and Q receive pointers are multiples of 16, and the element form with the send pointers
// one base element and the receive pointers two base elements further — but for the 16-B pairs, whose element is
// the 16-B granule at any address.
static void matrix_layouts() {
  const struct { int code, elem; } types[13] = {{1, 1}, {2, 2}, {3, 2}, {4, 1}, {5, 4}, {6, 8}, {7, 4}, {8, 8},
                                                {0x103, 4}, {0x105, 8}, {0x106, 16}, {0x107, 8}, {0x108, 16}};
  for (const auto& t : types) {
    const TypeForm old = basic(t.code);
    const TypeForm f = vec(3, 32 / t.elem, 48 / t.elem, old);
    CHECK(reduce_dt_elem_bytes(f) == t.elem);
    CHECK(f.size() * f.bsz == 96 && f.extent() * f.bsz == 128);
    uint32_t elog = 0;
    while ((1 << elog) < t.elem) elog++;
    for (int64_t items : {3, 43, 171}) {
      SideBytes lay;
      std::string err;
      CHECK(reduce_dt_layout(f, items, &lay, &err));
      CHECK(lay.total() == 96 * items);
      for (int P = 2; P <= 8; P++) {
        uint64_t at0[16], at12[16];  // P send pointers, then P receive pointers
        for (int i = 0; i < 2 * P; i++) {
          at0[i] = 0x7f0000001000ull + 0x4000ull * (uint64_t)i;
          at12[i] = at0[i] + (uint64_t)((i < P ? 1 : 2) * f.bsz);
        }
        CHECK(reduce_dt_granule_log(lay, t.elem, at0, 2 * P) == 4);
        CHECK(reduce_dt_granule_log(lay, t.elem, at0, P + 1) == 4);  // Reduce: the root's receive pointer only
        CHECK(reduce_dt_granule_log(lay, t.elem, at12, 2 * P) == elog);
        CHECK(reduce_dt_granule_log(lay, t.elem, at12, P + 1) == elog);
      }
      walk(f, items, 4, "the matrix layout, 16 B");
      walk(f, items, elog, "the matrix layout, elements");
    }
  }
}

// Block r of Reduce_scatter: granule i of its range, read at the rebased pointer, is granule i of a layout of
// recvcounts[r] items at the receive buffer's own origin
static void ranges(const TypeForm& f, uint32_t glog, const char* what) {
  const int64_t rc[4] = {2, 0, 3, 1};
  SideBytes all;
  std::string err;
  CHECK(reduce_dt_layout(f, 6, &all, &err));
  IndexedSide side, own;
  int64_t ngran = 0, n = 0;
  const IdxEnt* tab = all.irr ? all.irr->tab.data() : nullptr;
  CHECK(plan_reduce_dt(all, glog, tab, &side, &ngran, &err) == kTypeOk);
  int64_t item0 = 0, covered = 0;
  for (int r = 0; r < 4; item0 += rc[r], r++) {
    const DtRange g = reduce_dt_range(item0, rc[r], f.size() * f.bsz, f.extent() * f.bsz, glog);
    CHECK(g.q0 == covered);
    covered += g.nq;
    if (rc[r] == 0) {
      CHECK(g.nq == 0);
      continue;
    }
    SideBytes mine;
    CHECK(reduce_dt_layout(f, rc[r], &mine, &err));
    CHECK(plan_reduce_dt(mine, glog, tab, &own, &n, &err) == kTypeOk);
    CHECK(n == g.nq);
    int bad = 0;
    for (uint32_t i = 0; i < g.nq; i++)
      bad += reduce_dt_offset(side, g.q0 + i, glog) - g.rebase != reduce_dt_offset(own, i, glog);
    if (bad) printf("  %s rank %d: %d granules off\n", what, r, bad);
    CHECK(bad == 0);
  }
  CHECK(covered == ngran);
}

static void forms() {
  const TypeForm INT = basic(5), FLT = basic(7), I2 = basic(0x105);
  CHECK(same_form(vec(6, 2, 5, INT), vec(6, 2, 5, INT)));
  CHECK(!same_form(vec(6, 2, 5, INT), vec(6, 2, 6, INT)));
  CHECK(!same_form(vec(6, 2, 5, INT), vec(6, 2, 5, FLT)));
  CHECK(!same_form(vec(3, 2, 5, INT), vec(3, 1, 5, I2)));  // the same blocks, of pairs
  CHECK(same_form(indexed({2, 1}, {9, 4}, INT), indexed({2, 1}, {9, 4}, INT)));
  CHECK(!same_form(indexed({2, 1}, {9, 4}, INT), indexed({1, 2}, {9, 4}, INT)));
  CHECK(!same_form(indexed({5, 7}, {9, 0}, INT), vec(4, 3, 7, INT)));
  CHECK(same_form(indexed({2, 2}, {0, 5}, INT), vec(2, 2, 5, INT)));  // a regular list IS the Vector
}

int main() {
  offsets();
  granule();
  matrix_layouts();
  forms();
  ranges(vec(4, 3, 7, basic(5)), 2, "Vector(4,3,7) INT");
  ranges(vec(9, 4, 10, basic(8)), 4, "Vector(9,4,10) DOUBLE 16 B");
  ranges(vec(4, 3, 3, basic(5)), 2, "contiguous");
  ranges(indexed({2, 2, 2}, {1, 11, 5}, basic(5), true), 2, "Hindexed, lb = 1");
  ranges(indexed({2}, {3}, basic(5)), 2, "one block at lb = 3");
  if (fails) {
    printf("reduce_dt_plan_test: %d checks FAILED\n", fails);
    return 1;
  }
  printf("reduce_dt_plan_test: ok\n");
  return 0;
}
