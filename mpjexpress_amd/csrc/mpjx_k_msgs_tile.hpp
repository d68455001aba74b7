// mpjx_k_msgs_tile.hpp — what one workgroup of k_msgs (mpjx_k_msgs.hip) and of k_msgs_pool (mpjx_k_msgs_pool.hip)
// does with one tile of one segment: the tile shapes, the bytes kind and the granule kind. The two kernels differ
// only in where block g finds its segment (a table in the kernel argument; a slot of the device pool), so the
// per-lane code lives here once. Device code: included by those two files only.
#pragma once
#include "mpjx_kernels.hpp"
#include "mpjx_msgs_plan.hpp"

namespace mpjx {

namespace {

template <bool NT>
struct MsgsTile {
  static constexpr int TH = NT ? 512 : 256;
  static constexpr int U = NT ? 1 : 4;
  static constexpr int64_t tile = TH * U;
};

using gv4u = __attribute__((address_space(1))) v4u;
using gu8 = __attribute__((address_space(1))) unsigned char;
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

template <bool NT, class P>
__device__ __forceinline__ auto ldn(const P* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT, class P, class V>
__device__ __forceinline__ void stn(P* p, V v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// The 16 bytes that start sh bytes (1..15, uniform) into the 32 bytes {lo, hi}
__device__ __forceinline__ v4u shift16(v4u lo, v4u hi, unsigned sh) {
  const unsigned w[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  const unsigned q = sh >> 2, b = sh & 3u;
  unsigned x[5];
#pragma unroll
  for (int k = 0; k < 5; k++) x[k] = q == 0 ? w[k] : q == 1 ? w[k + 1] : q == 2 ? w[k + 2] : w[k + 3];
  v4u r;
#pragma unroll
  for (int k = 0; k < 4; k++) r[k] = __builtin_amdgcn_alignbyte(x[k + 1], x[k], b);
  return r;
}

template <bool NT>
__device__ __forceinline__ void bytes_tile(const MsgSeg& m, int64_t x, int64_t last) {
  constexpr int TH = MsgsTile<NT>::TH;
  constexpr int U = MsgsTile<NT>::U;
  constexpr int64_t TILE = MsgsTile<NT>::tile;
  const uint64_t src = m.g.s.r.base, dst = m.g.d.r.base;
  const MoveGeom gm = move_geom(dst, m.bytes);
  // every whole vector's source starts sh bytes into an aligned 16-B granule, sh uniform per segment; both
  // granules hold at least one byte of the message, so neither load leaves the pages the message touches
  const unsigned sh = (unsigned)((src - gm.da) & 15u);
  if (sh == 0) {
    v4u v[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const MsgVec mv = msg_bytes_vec(m, gm, x, TILE, u * TH + threadIdx.x);
      if (mv.on) v[u] = ldn<NT>((const gv4u*)mv.src);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const MsgVec mv = msg_bytes_vec(m, gm, x, TILE, u * TH + threadIdx.x);
      if (mv.on) stn<NT>((gv4u*)mv.dst, v[u]);
    }
  } else {
    v4u a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const MsgVec mv = msg_bytes_vec(m, gm, x, TILE, u * TH + threadIdx.x);
      if (mv.on) {
        const gv4u* p = (const gv4u*)(mv.src - sh);
        a[u] = ldn<NT>(p);
        b[u] = ldn<NT>(p + 1);
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const MsgVec mv = msg_bytes_vec(m, gm, x, TILE, u * TH + threadIdx.x);
      if (mv.on) stn<NT>((gv4u*)mv.dst, shift16(a[u], b[u], sh));
    }
  }
  const gu8* S = (const gu8*)src;
  gu8* D = (gu8*)dst;
  if (x == 0)
    for (int64_t k = threadIdx.x; k < gm.head; k += TH) D[k] = S[k];
  if (x == last)
    for (int64_t k = gm.ts + threadIdx.x; k < m.bytes; k += TH) D[k] = S[k];
}

template <bool NT, int GLOG>
__device__ __forceinline__ void granule_tile(const IndexedSeg& sg, uint32_t x) {
  constexpr int TH = MsgsTile<NT>::TH;
  constexpr int U = MsgsTile<NT>::U;
  using T = typename Granule<GLOG>::type;
  using GT = __attribute__((address_space(1))) T;
  // x < 2^32 / (TH * U) tiles: q0 + u * TH + t stays below 2^32 + TH * U, computed in 64 bits
  const uint64_t q0 = (uint64_t)x * (TH * U) + threadIdx.x;
  T v[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const uint64_t q = q0 + (uint64_t)u * TH;
    if (q < sg.ngran) v[u] = ldn<NT>((const GT*)indexed_addr(sg.s, (uint32_t)q, GLOG));
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    const uint64_t q = q0 + (uint64_t)u * TH;
    if (q < sg.ngran) stn<NT>((GT*)indexed_addr(sg.d, (uint32_t)q, GLOG), v[u]);
  }
}

// Tile x of the `ntiles` tiles of segment m (uniform per workgroup: the branch on the kind is scalar)
template <bool NT>
__device__ __forceinline__ void msgs_tile(const MsgSeg& m, uint32_t x, uint32_t ntiles) {
  if (m.kind == kMsgBytes) {
    bytes_tile<NT>(m, x, (int64_t)ntiles - 1);
    return;
  }
  switch (m.g.glog) {
    case 0: granule_tile<NT, 0>(m.g, x); break;
    case 1: granule_tile<NT, 1>(m.g, x); break;
    case 2: granule_tile<NT, 2>(m.g, x); break;
    case 3: granule_tile<NT, 3>(m.g, x); break;
    default: granule_tile<NT, 4>(m.g, x); break;
  }
}

static_assert(MsgsTile<false>::tile == kStridedTile && MsgsTile<true>::tile == kStridedTileNT,
              "the planner's tiles are the kernel's");

}  // namespace

}  // namespace mpjx
