// mpjx_k_transpose.hip — k_transpose: the element transposes among the strided moves, up to kTransposeMax
// segments in one launch (mpjx_transpose_plan.hpp: the eligibility test, the descriptor and the geometry).
//   - A segment is a strided side X of R rows x C columns of one granule (1, 2, 4, 8 or 16 bytes) and a
//     contiguous side Y that holds the same granules column by column: packed granule q = c * R + r.
//   - The grid is the SUM of the segments' tiles (TransposeTable::tile0, as k_strided): block g searches the
//     prefix for its (segment, tile); a table of one segment skips the search. Tile index -> (tile row, tile
//     column) is one multiply-high by a per-segment reciprocal (FastDiv): no integer division on the device.
//   - One workgroup of 256 lanes moves one T x T tile through LDS (T = 64 up to 4-byte granules, 32 above):
//     gather (X -> Y) loads with neighbouring lanes on neighbouring columns of X, stores the tile to LDS,
//     waits at the barrier, then reads LDS transposed and stores with neighbouring lanes on neighbouring rows,
//     which are neighbouring granules of Y. Scatter (Y -> X) is the mirror image. Both global sides of every
//     tile are accessed with consecutive lanes on consecutive granules.
//   - The LDS pitch is padded by one granule (at least 4 bytes): the transposed reads are conflict-free for
//     every granule size (the arithmetic is in the plan header).
//   - Edge tiles are predicated slot by slot: no byte outside Y's run or outside X's R x C granules is loaded or
//     stored, and the gaps between X's rows keep their contents.
// Loads and stores go through global-address-space pointers, with the default cache policy: a row of X is read
// (or written) by T / granules-per-line neighbouring tiles, and the L2 is what joins them. No non-temporal
// form exists; none has been measured ahead.
#include <stdlib.h>

#include "mpjx_kernels.hpp"
#include "mpjx_transpose_plan.hpp"

namespace mpjx {

namespace {

using v2u = unsigned int __attribute__((ext_vector_type(2)));

template <int GLOG>
struct TrGranule;
template <>
struct TrGranule<0> { using type = unsigned char; };
template <>
struct TrGranule<1> { using type = unsigned short; };
template <>
struct TrGranule<2> { using type = unsigned int; };
template <>
struct TrGranule<3> { using type = v2u; };
template <>
struct TrGranule<4> { using type = v4u; };

template <int GLOG>
__device__ __forceinline__ void transpose_tile(const TransposeSeg& sg, uint32_t x, unsigned char* lds) {
  using T = typename TrGranule<GLOG>::type;
  using GT = __attribute__((address_space(1))) T;
  constexpr uint32_t side = GLOG <= 2 ? 64 : 32;
  constexpr int N = (int)(side * side / kTrLanes);  // slots per lane: 16 or 4
  TransposeSeg t = sg;
  t.glog = GLOG;  // a constant for the geometry below
  const bool gather = t.gather != 0;
  T v[N];
  // first walk: along the source side
#pragma unroll
  for (int u = 0; u < N; u++) {
    const TrSlot s = tr_slot(t, x, (uint32_t)u * kTrLanes + threadIdx.x, gather);
    if (s.on) v[u] = *(const GT*)(gather ? tr_addr_x(t, s.r, s.c) : tr_addr_y(t, s.r, s.c));
  }
#pragma unroll
  for (int u = 0; u < N; u++) {
    const TrSlot s = tr_slot(t, x, (uint32_t)u * kTrLanes + threadIdx.x, gather);
    if (s.on) *(T*)(lds + tr_lds(t, s)) = v[u];
  }
  __syncthreads();
  // second walk: along the destination side
#pragma unroll
  for (int u = 0; u < N; u++) {
    const TrSlot s = tr_slot(t, x, (uint32_t)u * kTrLanes + threadIdx.x, !gather);
    if (s.on) v[u] = *(const T*)(lds + tr_lds(t, s));
  }
#pragma unroll
  for (int u = 0; u < N; u++) {
    const TrSlot s = tr_slot(t, x, (uint32_t)u * kTrLanes + threadIdx.x, !gather);
    if (s.on) *(GT*)(gather ? tr_addr_y(t, s.r, s.c) : tr_addr_x(t, s.r, s.c)) = v[u];
  }
}

}  // namespace

// ONE: a table of one segment (every P = 1 call) skips the search, as k_strided's does
template <bool ONE>
__global__ __launch_bounds__(kTrLanes) void k_transpose(TransposeTable t) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kTrLdsBytes];
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
  const TransposeSeg& sg = t.seg[c];
  const uint32_t x = ONE ? g : g - t.tile0[c];  // tile0[0] = 0
  switch (sg.glog) {  // uniform per block
    case 0: transpose_tile<0>(sg, x, lds); break;
    case 1: transpose_tile<1>(sg, x, lds); break;
    case 2: transpose_tile<2>(sg, x, lds); break;
    case 3: transpose_tile<3>(sg, x, lds); break;
    default: transpose_tile<4>(sg, x, lds); break;
  }
}

hipError_t launch_transpose(const std::vector<TransposeSeg>& segs, hipStream_t s) {
  if (segs.empty()) return hipSuccess;
  std::vector<TransposeTable> tabs;
  plan_transpose_tables(segs, &tabs);
  for (const TransposeTable& t : tabs) {
    const unsigned grid = t.tile0[t.n];
    if (t.n == 1) hipLaunchKernelGGL((k_transpose<true>), dim3(grid), dim3(kTrLanes), 0, s, t);
    else hipLaunchKernelGGL((k_transpose<false>), dim3(grid), dim3(kTrLanes), 0, s, t);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace mpjx
