// mpjx_k_strided.hip — k_strided: the packed byte streams of up to kStridedMax strided moves in one launch,
// for the block moves with a derived datatype (Contiguous / Vector) on either side (mpjx_alltoallv_dt).
//   - A segment is a source layout and a destination layout of equal packed length (StridedSeg,
//     mpjx_strided_plan.hpp): items `eb` bytes apart, `nb` blocks per item `sb` bytes apart. A contiguous
//     side is one block. The packed stream is cut into granules — the largest power of two <= 16 B that
//     divides both sides' block bytes, strides, extents and bases, chosen per segment on the host — so a
//     granule never straddles a block on either side and every load and store is naturally aligned.
//   - The grid is the SUM of the segments' tiles (StridedTable::tile0, as k_moves): block g searches the
//     prefix for its (segment, tile); no block exists for a tile that does not.
//   - Lane t of a tile takes packed granule x * tile + u * lanes + t: neighbouring lanes take neighbouring
//     granules of a block, so blocks of 64 B or more are read and written in whole coalesced pieces. Each
//     lane turns its granule index into a source and a destination address with two divisions per side by
//     per-segment constants (granules per block, blocks per item), done as 32 x 64-bit multiply-highs with
//     reciprocals from the host (FastDiv): no integer division on the device.
//   - Only bytes inside destination blocks are stored; gaps keep their contents.
// Loads and stores go through global-address-space pointers, and the tile shapes and the streaming
// threshold are k_moves' (see there): 256 lanes x 4 granules with the default cache policy; from 64 MiB per
// call 512 lanes x 1 granule, non-temporal.
#include <stdlib.h>

#include "mpjx_kernels.hpp"
#include "mpjx_strided_plan.hpp"

namespace mpjx {

namespace {

template <bool NT>
struct StridedTile {
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

template <bool NT, int GLOG>
__device__ __forceinline__ void strided_tile(const StridedSeg& sg, uint32_t x) {
  constexpr int TH = StridedTile<NT>::TH;
  constexpr int U = StridedTile<NT>::U;
  using T = typename Granule<GLOG>::type;
  using GT = __attribute__((address_space(1))) T;
  // x < 2^32 / (TH * U) tiles: q0 + u * TH + t stays below 2^32 + TH * U, computed in 64 bits
  const uint64_t q0 = (uint64_t)x * (TH * U) + threadIdx.x;
  T v[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const uint64_t q = q0 + (uint64_t)u * TH;
    if (q < sg.ngran) {
      const GT* p = (const GT*)strided_addr(sg.s, (uint32_t)q, GLOG);
      if constexpr (NT) v[u] = __builtin_nontemporal_load(p);
      else v[u] = *p;
    }
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    const uint64_t q = q0 + (uint64_t)u * TH;
    if (q < sg.ngran) {
      GT* p = (GT*)strided_addr(sg.d, (uint32_t)q, GLOG);
      if constexpr (NT) __builtin_nontemporal_store(v[u], p);
      else *p = v[u];
    }
  }
}

}  // namespace

// ONE: a table of one segment (every P = 1 call) skips the search, as k_moves' does: the block's first load
// waits for one round of kernel-argument loads instead of two.
template <bool NT, bool ONE>
__global__ __launch_bounds__(StridedTile<NT>::TH) void k_strided(StridedTable t) {
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
  const StridedSeg& sg = t.seg[c];
  const uint32_t x = ONE ? g : g - t.tile0[c];  // tile0[0] = 0
  switch (sg.glog) {  // uniform per block
    case 0: strided_tile<NT, 0>(sg, x); break;
    case 1: strided_tile<NT, 1>(sg, x); break;
    case 2: strided_tile<NT, 2>(sg, x); break;
    case 3: strided_tile<NT, 3>(sg, x); break;
    default: strided_tile<NT, 4>(sg, x); break;
  }
}

static_assert(StridedTile<false>::gran == kStridedTile && StridedTile<true>::gran == kStridedTileNT,
              "the planner's tiles are the kernel's");

// MPJX_STRIDED_NT_MIN_MIB (read per call) moves the streaming threshold, for timing the two forms on the same
// bytes (tools/bench_strided.py --policies)
static int64_t stream_bytes() {
  const char* e = getenv("MPJX_STRIDED_NT_MIN_MIB");
  const long m = e ? atol(e) : 0;
  return m > 0 ? (int64_t)m << 20 : kStridedStreamBytes;
}

hipError_t launch_strided(const std::vector<StridedSeg>& segs, hipStream_t s) {
  int64_t total = 0;
  for (const StridedSeg& m : segs) total += (int64_t)m.ngran << m.glog;
  if (total == 0) return hipSuccess;
  const bool nt = total >= stream_bytes();
  std::vector<StridedTable> tabs;
  plan_strided_tables(segs, nt ? kStridedTileNT : kStridedTile, &tabs);
  for (const StridedTable& t : tabs) {
    const unsigned grid = t.tile0[t.n];
    if (nt && t.n == 1) hipLaunchKernelGGL((k_strided<true, true>), dim3(grid), dim3(StridedTile<true>::TH), 0, s, t);
    else if (nt) hipLaunchKernelGGL((k_strided<true, false>), dim3(grid), dim3(StridedTile<true>::TH), 0, s, t);
    else if (t.n == 1) hipLaunchKernelGGL((k_strided<false, true>), dim3(grid), dim3(StridedTile<false>::TH), 0, s, t);
    else hipLaunchKernelGGL((k_strided<false, false>), dim3(grid), dim3(StridedTile<false>::TH), 0, s, t);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace mpjx
