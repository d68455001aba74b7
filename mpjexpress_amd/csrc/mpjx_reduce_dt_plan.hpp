// mpjx_reduce_dt_plan.hpp — host-side planning of the reductions on derived datatypes (mpjx_reduce_dt,
// mpjx_allreduce_dt, mpjx_reduce_scatter_dt, mpjx_scan_dt) and the argument block of their kernel, k_pway_dt
// (mpjx_kernels_dt.hpp). No HIP include: plain C++17, compiled, tested and sanitized on the CPU
// (tests/cpp/reduce_dt_plan_test.cpp); the kernel includes the same header, so the offsets the test walks
// are the offsets the kernel computes.
//
// A reduction takes ONE datatype for both buffers, so packed granule q of every rank's send buffer and of every
// receive buffer lies at the same byte OFFSET from its buffer's position. The layout is therefore planned once,
// at base 0 (plan_side with buf = 0: item k at k * extent, lb not subtracted), as an IndexedSide whose address
// function — strided_addr for a regular layout, indexed_addr for an irregular one — returns that offset; the
// kernel adds it to each of the P operand pointers and to each output pointer.
//   granule  16 B where the rule of strided_granule_log / IrrLayout::amask gives it over the layout's block
//            bytes, strides, extents and offsets AND over all P send and all receive pointers; otherwise one
//            element of the reduction (one base element, or one (value, index) pair). Blocks hold whole
//            elements, so a granule of either size never straddles a block.
//   range    a launch covers packed granules [q0, q0 + nq) of the layout. Reduce_scatter's block r is the
//            range of items [off_r, off_r + recvcounts[r]) with rank r's receive pointer moved back by
//            off_r * extent bytes, so that the block's first item lands on the receive buffer's own origin.
#pragma once
#include <string.h>

#include "mpjx_indexed_plan.hpp"

namespace mpjx {

constexpr int kDtMaxP = 8;  // operands of one k_pway_dt launch (MAXP of mpjx_kernels.hpp)

// The kernel's argument block
struct PwayDtArgs {
  const void* in[kDtMaxP];
  void* out[kDtMaxP];
  IndexedSide lay;   // the shared layout at base 0; lay.tab = the type's device table (irregular) or nullptr
  uint32_t q0 = 0;   // first packed granule of the launch
  uint32_t nq = 0;   // granules of the launch
  int root = 0;      // K_MST root
  int nrep = 1;      // K_FOLD / K_MST: the result is stored to out[0..nrep)
};

// The layout of `items` items of `f` at base 0. False with *err set as plan_side.
inline bool reduce_dt_layout(const TypeForm& f, int64_t items, SideBytes* out, std::string* err) {
  return plan_side(f, 0, items, 0, out, err, "count");
}

// Bytes per element of the reduction: one base element, or one pair
inline int reduce_dt_elem_bytes(const TypeForm& f) { return f.pair ? 2 * f.bsz : f.bsz; }

// log2 of the granule: 4 where the layout and every one of the `n` pointers allow 16-B accesses, else the
// element's (elem_bytes a power of two <= 16)
inline uint32_t reduce_dt_granule_log(const SideBytes& lay, int elem_bytes, const uint64_t* ptrs, int n) {
  uint64_t mask = side_align_mask(lay);
  for (int i = 0; i < n; i++) mask |= ptrs[i];
  if ((mask & 15u) == 0) return 4;
  uint32_t g = 0;
  while ((1 << g) < elem_bytes) g++;
  return g;
}

// The kernel's descriptor of `lay` in granules of 2^glog bytes, and the layout's granule count.
// kTypeErrUnsupported with *err set for 2^32 granules or more.
inline int plan_reduce_dt(const SideBytes& lay, uint32_t glog, const IdxEnt* tab, IndexedSide* out, int64_t* ngran,
                          std::string* err) {
  const int64_t n = lay.total() >> glog;
  if (n > kStridedMaxGran) {
    *err = "a reduction of " + std::to_string(lay.total()) + " bytes in granules of " + std::to_string(1 << glog) +
           " B exceeds 2^32 - 1 granules";
    return kTypeErrUnsupported;
  }
  out->tab = lay.irr ? tab : nullptr;
  out->r.base = lay.base;
  out->r.sb = (uint64_t)lay.sb;
  out->r.eb = (uint64_t)lay.eb;
  const int64_t per = (lay.irr ? lay.irr->size : lay.bb) >> glog;  // granules per item (irregular) or block
  out->r.bbg = fast_div((uint32_t)std::max<int64_t>(per, 1));
  out->r.nb = fast_div((uint32_t)std::min<int64_t>(std::max<int64_t>(lay.nb, 1), kStridedMaxGran));
  *ngran = n;
  return kTypeOk;
}

// The byte offset of packed granule q from a buffer's position: the one address function of the kernel
MPJX_HD inline uint64_t reduce_dt_offset(const IndexedSide& lay, uint32_t q, uint32_t glog) {
  return indexed_addr(lay, q, glog);
}

// Reduce_scatter's block of items [item0, item0 + nitems) of a type of `size_bytes` packed bytes and
// `extent_bytes` extent per item: its granule range, and how far the receiving rank's pointer moves back.
struct DtRange {
  uint32_t q0, nq;
  uint64_t rebase;  // bytes subtracted from the receive pointer
};
inline DtRange reduce_dt_range(int64_t item0, int64_t nitems, int64_t size_bytes, int64_t extent_bytes, uint32_t glog) {
  DtRange r;
  r.q0 = (uint32_t)((item0 * size_bytes) >> glog);
  r.nq = (uint32_t)((nitems * size_bytes) >> glog);
  r.rebase = (uint64_t)(item0 * extent_bytes);
  return r;
}

// Two types that normalise to the same form: the same blocks at the same offsets, whatever their codes (rank
// threads create their own types)
inline bool same_form(const TypeForm& a, const TypeForm& b) {
  if (a.base != b.base || a.bsz != b.bsz || a.pair != b.pair || !a.irr != !b.irr) return false;
  if (a.lb() != b.lb() || a.ub() != b.ub()) return false;  // an explicit extent moves the items
  if (!a.irr) return a.nblocks == b.nblocks && a.blocklen == b.blocklen && a.stride == b.stride;
  const IrrLayout &x = *a.irr, &y = *b.irr;
  return x.size == y.size && x.lb == y.lb && x.ub == y.ub && x.tab.size() == y.tab.size() &&
         memcmp(x.tab.data(), y.tab.data(), x.tab.size() * sizeof(IdxEnt)) == 0;
}

}  // namespace mpjx
