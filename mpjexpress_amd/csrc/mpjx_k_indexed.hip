// mpjx_k_indexed.hip — k_indexed: the packed byte streams of up to kIndexedMax moves in one launch, where at
// least one side of a move is an irregular layout (Hvector / Indexed / Hindexed, mpjx_indexed_plan.hpp).
// Shaped like k_strided (see there for the tiles, the prefix table of the grid, the granule and the cache
// policies): one lane moves one granule, neighbouring lanes take neighbouring granules of the packed stream.
//   - Per segment each side is either k_strided's regular side or an irregular one: the origin of item 0,
//     the item extent, the granules per item (FastDiv), the block count and a pointer to the type's device
//     table of {byte offset, packed-byte prefix} per block, 16 B each. The kind is uniform per segment, so
//     the branch on it is scalar.
//   - Packed granule q of an irregular side lies in item q / gpi; the block of the remainder's packed byte is
//     the last table entry whose prefix does not exceed it: a binary search, one 16-B load per probe
//     (indexed_addr). The granule divides every block offset and length, so no access is misaligned and none
//     straddles a block.
//   - Two forms of the search. DIRECT: every lane probes the device table; the table of a type in use sits
//     in L2. Correct at any table size. LDS: the workgroup first copies the tables of its segment's
//     irregular sides into LDS (kIndexedLdsBlocks entries per side at most) and the lanes probe there; a
//     side with a larger table is searched directly. launch_indexed takes the LDS form for a launch table
//     that has a side of at most lds_max_blocks() blocks: by default every table the LDS form can hold
//     (DESIGN.md §4 "Indexed moves" has the measurement behind that).
#include <stdlib.h>

#include "mpjx_kernels.hpp"
#include "mpjx_indexed_plan.hpp"

namespace mpjx {

namespace {

constexpr int kIndexedLdsBlocks = 512;  // entries per side the LDS form can hold: 2 x 8 KiB per workgroup

template <bool NT>
struct IndexedTile {
  static constexpr int TH = NT ? 512 : 256;
  static constexpr int U = NT ? 1 : 4;
  static constexpr int64_t gran = TH * U;
};

using v2u = unsigned int __attribute__((ext_vector_type(2)));

template <int GLOG>
struct Granule;
template <>
struct Granule<0> { using type = unsigned char; };
template <>
struct Granule<1> { using type = unsigned short; };
template <>
struct Granule<2> { using type = unsigned int; };
template <>
struct Granule<3> { using type = v2u; };
template <>
struct Granule<4> { using type = v4u; };

// `lds`: this side's copy of the table, or nullptr to search the device table
template <int GLOG>
__device__ __forceinline__ uint64_t side_addr(const IndexedSide& x, const IdxEnt* lds, uint32_t q) {
  if (x.tab && lds) {
    typedef __attribute__((address_space(3))) const IdxEnt LE;  // ds_read, not a flat load
    LE* p = (LE*)lds;
    return irregular_addr(x, q, GLOG, [p](uint32_t i) { return IdxEnt{p[i].off, p[i].pre}; });
  }
  return indexed_addr(x, q, GLOG);
}

template <bool NT, int GLOG>
__device__ __forceinline__ void indexed_tile(const IndexedSeg& sg, uint32_t x, const IdxEnt* ls, const IdxEnt* ld) {
  constexpr int TH = IndexedTile<NT>::TH;
  constexpr int U = IndexedTile<NT>::U;
  using T = typename Granule<GLOG>::type;
  using GT = __attribute__((address_space(1))) T;
  // x < 2^32 / (TH * U) tiles: q0 + u * TH + t stays below 2^32 + TH * U, computed in 64 bits
  const uint64_t q0 = (uint64_t)x * (TH * U) + threadIdx.x;
  T v[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const uint64_t q = q0 + (uint64_t)u * TH;
    if (q < sg.ngran) {
      const GT* p = (const GT*)side_addr<GLOG>(sg.s, ls, (uint32_t)q);
      if constexpr (NT) v[u] = __builtin_nontemporal_load(p);
      else v[u] = *p;
    }
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    const uint64_t q = q0 + (uint64_t)u * TH;
    if (q < sg.ngran) {
      GT* p = (GT*)side_addr<GLOG>(sg.d, ld, (uint32_t)q);
      if constexpr (NT) __builtin_nontemporal_store(v[u], p);
      else *p = v[u];
    }
  }
}

// The workgroup's copy of one side's table, or nullptr where the side is regular or its table too large
template <int TH>
__device__ __forceinline__ const IdxEnt* stage(const IndexedSide& x, IdxEnt* lds, uint32_t cap) {
  if (!x.tab || x.r.nb.d > cap) return nullptr;
  for (uint32_t i = threadIdx.x; i < x.r.nb.d; i += TH) lds[i] = idx_entry(x.tab, i);
  return lds;
}

}  // namespace

// ONE: a table of one segment (every P = 1 call) skips the search for the segment, as k_strided's does.
template <bool NT, bool ONE, bool LDS>
__global__ __launch_bounds__(IndexedTile<NT>::TH) void k_indexed(IndexedTable t, uint32_t cap) {
  const unsigned g = blockIdx.x;
  int c = 0;  // the segment whose tiles hold block g: tile0[c] <= g < tile0[c + 1]
  if constexpr (!ONE) {
    int hi = t.n;
    while (hi - c > 1) {
      const int mid = (c + hi) >> 1;
      if (t.tile0[mid] <= g) c = mid;
      else hi = mid;
    }
  }
  const IndexedSeg& sg = t.seg[c];
  const uint32_t x = ONE ? g : g - t.tile0[c];  // tile0[0] = 0
  const IdxEnt *ls = nullptr, *ld = nullptr;
  if constexpr (LDS) {
    __shared__ IdxEnt lds[2][kIndexedLdsBlocks];
    ls = stage<IndexedTile<NT>::TH>(sg.s, lds[0], cap);  // cap <= kIndexedLdsBlocks
    ld = stage<IndexedTile<NT>::TH>(sg.d, lds[1], cap);
    __syncthreads();
  }
  switch (sg.glog) {  // uniform per block
    case 0: indexed_tile<NT, 0>(sg, x, ls, ld); break;
    case 1: indexed_tile<NT, 1>(sg, x, ls, ld); break;
    case 2: indexed_tile<NT, 2>(sg, x, ls, ld); break;
    case 3: indexed_tile<NT, 3>(sg, x, ls, ld); break;
    default: indexed_tile<NT, 4>(sg, x, ls, ld); break;
  }
}

static_assert(IndexedTile<false>::gran == kStridedTile && IndexedTile<true>::gran == kStridedTileNT,
              "the planner's tiles are the kernel's");

// MPJX_STRIDED_NT_MIN_MIB (read per call) moves the streaming threshold, as for k_strided.
static int64_t stream_bytes() {
  const char* e = getenv("MPJX_STRIDED_NT_MIN_MIB");
  const long m = e ? atol(e) : 0;
  return m > 0 ? (int64_t)m << 20 : kStridedStreamBytes;
}

// The largest table (blocks) searched in LDS. MPJX_INDEXED_LDS_MAX_BLOCKS (read per call) moves it, for
// timing the two forms on the same bytes (tools/bench_indexed.py --forms): 0 turns the LDS form off. The
// default is all the LDS form can hold: at 256 and 512 blocks it took 0.63 - 0.96 of the direct form's time
// (0.63 - 0.84 but for the 8-B scatters), every row outside both forms' spread (DESIGN.md §4 "Indexed moves").
constexpr int kIndexedLdsDefault = kIndexedLdsBlocks;
static uint32_t lds_max_blocks() {
  const char* e = getenv("MPJX_INDEXED_LDS_MAX_BLOCKS");
  const long m = e ? atol(e) : kIndexedLdsDefault;
  return (uint32_t)std::min<long>(std::max<long>(m, 0), kIndexedLdsBlocks);
}

template <bool NT, bool ONE>
static void launch_form(const IndexedTable& t, bool lds, uint32_t cap, hipStream_t s) {
  const unsigned grid = t.tile0[t.n];
  if (lds) hipLaunchKernelGGL((k_indexed<NT, ONE, true>), dim3(grid), dim3(IndexedTile<NT>::TH), 0, s, t, cap);
  else hipLaunchKernelGGL((k_indexed<NT, ONE, false>), dim3(grid), dim3(IndexedTile<NT>::TH), 0, s, t, cap);
}

hipError_t launch_indexed(const std::vector<IndexedSeg>& segs, hipStream_t s) {
  int64_t total = 0;
  for (const IndexedSeg& m : segs) total += (int64_t)m.ngran << m.glog;
  if (total == 0) return hipSuccess;
  const bool nt = total >= stream_bytes();
  const uint32_t cap = lds_max_blocks();
  std::vector<IndexedTable> tabs;
  plan_indexed_tables(segs, nt ? kStridedTileNT : kStridedTile, &tabs);
  for (const IndexedTable& t : tabs) {
    bool lds = false;
    for (int c = 0; c < t.n; c++)
      for (const IndexedSide* x : {&t.seg[c].s, &t.seg[c].d}) lds = lds || (x->tab && x->r.nb.d <= cap);
    if (nt && t.n == 1) launch_form<true, true>(t, lds, cap, s);
    else if (nt) launch_form<true, false>(t, lds, cap, s);
    else if (t.n == 1) launch_form<false, true>(t, lds, cap, s);
    else launch_form<false, false>(t, lds, cap, s);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace mpjx
