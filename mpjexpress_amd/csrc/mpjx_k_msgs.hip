// mpjx_k_msgs.hip — k_msgs: a batch of matched point-to-point messages of mixed layout kinds in ONE launch
// (mpjx_p2p.hip: what a Waitall of a halo exchange moves). DtMoves::launch spends one launch per kernel family;
// at halo sizes the fixed launch cost is the whole cost, so the kinds share a kernel here.
//   - The table (MsgsTable, mpjx_msgs_plan.hpp) holds up to kMsgsMax segments and the prefix of their tiles: the
//     grid is the SUM of the tiles and block g searches the prefix for its (segment, tile), as k_strided does.
//   - A segment's kind is uniform per workgroup, so the branch on it is scalar.
//   - bytes: both layouts contiguous at any pair of byte alignments: k_moves' destination-grid geometry. Every
//     whole destination vector is one aligned 16-B store, its source one aligned 16-B load or two combined by
//     v_alignbyte_b32; head and tail are byte stores by the first and the last tile, inside the message only.
//   - granule: either side regular or irregular; lane t takes packed granule x * tile + u * lanes + t and turns
//     it into a source and a destination address with indexed_addr (FastDiv reciprocals; an irregular side's
//     device table is searched where it lies: the LDS window of k_indexed is left out).
//   - Only bytes inside the destination's blocks, and only the sender's packed length, are stored.
// Tile shapes are the other move kernels': 256 lanes x 4 with the default cache policy, 512 lanes x 1 with
// non-temporal loads and stores from kStridedStreamBytes of batch payload (a threshold taken over from
// k_strided, not measured on this kernel).
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

}  // namespace

template <bool NT>
__global__ __launch_bounds__(MsgsTile<NT>::TH) void k_msgs(MsgsTable t) {
  const unsigned g = blockIdx.x;
  int c = 0, hi = t.n;  // the segment whose tiles hold block g: tile0[c] <= g < tile0[c + 1]
  while (hi - c > 1) {
    const int mid = (c + hi) >> 1;
    if (t.tile0[mid] <= g) c = mid;
    else hi = mid;
  }
  const MsgSeg& m = t.seg[c];
  const uint32_t x = g - t.tile0[c];
  if (m.kind == kMsgBytes) {  // uniform per block
    bytes_tile<NT>(m, x, (int64_t)(t.tile0[c + 1] - t.tile0[c]) - 1);
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

hipError_t launch_msgs(const std::vector<MsgSeg>& segs, hipStream_t s, int64_t* launches) {
  int64_t total = 0;
  for (const MsgSeg& m : segs) total += m.bytes > 0 ? m.bytes : 0;
  if (total == 0) return hipSuccess;
  const bool nt = total >= kStridedStreamBytes;
  std::vector<MsgsTable> tabs;
  plan_msgs_tables(segs, nt ? kStridedTileNT : kStridedTile, &tabs);
  for (const MsgsTable& t : tabs) {
    const unsigned grid = t.tile0[t.n];
    if (nt) hipLaunchKernelGGL((k_msgs<true>), dim3(grid), dim3(MsgsTile<true>::TH), 0, s, t);
    else hipLaunchKernelGGL((k_msgs<false>), dim3(grid), dim3(MsgsTile<false>::TH), 0, s, t);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (launches) ++*launches;
  }
  return hipSuccess;
}

}  // namespace mpjx
