// mpjx_k_wire.hip — k_wire: the typed <-> MPI.PACKED pairs of a claimed point-to-point batch in ONE launch per
// table (mpjx_p2p.hip routes them here; the table, the header checks and the per-lane arithmetic:
// mpjx_wire_plan.hpp). A typed send that meets a PACKED receive is packed into the receiver's image on the fly,
// a PACKED send that meets a typed receive is unpacked from the sender's image: layout, byte swap and header in
// one HBM pass, where a caller without it packs into scratch, sends the bytes and unpacks.
//   - The table holds up to kWireMax segments of either direction and any layout kind, and the prefix of their
//     tiles: the grid is the SUM of the tiles and block g searches the prefix for its (segment, tile), as k_msgs
//     does. Direction, granule and word size are uniform per workgroup, so those branches are scalar.
//   - The per-lane work is k_pack's: one granule of the packed stream per lane, neighbouring lanes on
//     neighbouring granules; the layout address from indexed_addr or the linear form (an irregular side's device
//     table is searched where it lies: no LDS form, as in k_msgs), the payload address pay + (q << glog); the
//     words byte-swapped in registers between the load and the store; global-address-space pointers.
//   - Pack: lane 0 of the segment's first block stores the 8 header bytes with one 8-byte store.
//   - Unpack: lane 0 of EVERY block of the segment loads the header (L2-resident after the first block), checks
//     it (wire_check_header) and broadcasts {err, n} through LDS before any payload byte is loaded. A bad header
//     ends the block: nothing is stored into the receive buffer. The segment's first block stores {code, n} into
//     the pair's result slot (pinned host memory, one ordinary 8-byte store from one lane), which the host reads
//     once the batch's completion event has passed. n comes from the header: granules wholly below n words move
//     whole, the one n cuts is moved word by word by the lane that owns it, those above are not touched.
// 256 lanes x 4 granules with the default cache policy; from the streaming threshold of the strided moves (64 MiB
// of batch payload, MPJX_STRIDED_NT_MIN_MIB) 512 lanes x 1 granule, non-temporal: a threshold taken over from
// k_strided, not measured on this kernel.
#include <stdlib.h>

#include "mpjx_kernels.hpp"
#include "mpjx_wire_plan.hpp"

namespace mpjx {

namespace {

template <bool NT>
struct WireTile {
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

template <int GLOG>
__device__ __forceinline__ uint64_t lay_addr(const WireSeg& a, uint32_t q) {
  if (a.lin) return a.lay.r.base + ((uint64_t)q << GLOG);  // uniform
  return indexed_addr(a.lay, q, GLOG);
}

// Tile x of segment a. Pack: every granule below a.ngran. Unpack: the granules wire_lane gives for n words.
template <bool UNPACK, bool NT, int GLOG, int WLOG>
__device__ __forceinline__ void wire_tile(const WireSeg& a, uint32_t x, int64_t n) {
  static_assert(GLOG >= WLOG, "a granule holds whole base words");
  constexpr int TH = WireTile<NT>::TH;
  constexpr int U = WireTile<NT>::U;
  constexpr int WS = 1 << WLOG;
  using T = typename Granule<GLOG>::type;
  using GT = __attribute__((address_space(1))) T;
  // whole granules: a.ngran of a pack; those wholly below n words of an unpack (never more than a.ngran)
  const uint64_t full = UNPACK ? ((uint64_t)n << WLOG) >> GLOG : (uint64_t)a.ngran;
  const uint64_t q0 = (uint64_t)x * (TH * U) + threadIdx.x;
  T v[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const uint64_t q = q0 + (uint64_t)u * TH;
    if (q < full) {
      const GT* p = (const GT*)(UNPACK ? a.pay + (q << GLOG) : lay_addr<GLOG>(a, (uint32_t)q));
      if constexpr (NT) v[u] = __builtin_nontemporal_load(p);
      else v[u] = *p;
    }
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    const uint64_t q = q0 + (uint64_t)u * TH;
    if (q < full) {
      const T w = swap_words<WS>(v[u]);
      GT* p = (GT*)(UNPACK ? lay_addr<GLOG>(a, (uint32_t)q) : a.pay + (q << GLOG));
      if constexpr (NT) __builtin_nontemporal_store(w, p);
      else *p = w;
    }
  }
  if constexpr (UNPACK && GLOG > WLOG) {  // the granule n cuts: its first r words, by the lane that owns it
    using W = typename Granule<WLOG>::type;
    using GW = __attribute__((address_space(1))) W;
    const uint32_t r = (uint32_t)((((uint64_t)n << WLOG) & ((1u << GLOG) - 1u)) >> WLOG);
    if (r != 0 && full >= q0 && full < (uint64_t)(x + 1) * (TH * U) && (full - q0) % TH == 0) {
      const GW* src = (const GW*)(a.pay + (full << GLOG));
      GW* dst = (GW*)lay_addr<GLOG>(a, (uint32_t)full);
      for (uint32_t k = 0; k < r; k++) dst[k] = swap_words<WS>(src[k]);
    }
  }
}

template <bool UNPACK, bool NT>
__device__ __forceinline__ void wire_arms(const WireSeg& a, uint32_t x, int64_t n) {
#define MPJX_WR(G, W)                        \
  case (G) * 4 + (W):                        \
    wire_tile<UNPACK, NT, G, W>(a, x, n);    \
    break;
  switch (a.glog * 4 + a.wlog) {  // uniform per workgroup; the planner keeps glog >= wlog
    MPJX_WR(0, 0) MPJX_WR(1, 0) MPJX_WR(2, 0) MPJX_WR(3, 0) MPJX_WR(4, 0)
    MPJX_WR(1, 1) MPJX_WR(2, 1) MPJX_WR(3, 1) MPJX_WR(4, 1)
    MPJX_WR(2, 2) MPJX_WR(3, 2) MPJX_WR(4, 2)
    MPJX_WR(3, 3) MPJX_WR(4, 3)
    default: break;
  }
#undef MPJX_WR
}

}  // namespace

template <bool NT>
__global__ __launch_bounds__(WireTile<NT>::TH) void k_wire(WireTable t) {
  typedef __attribute__((address_space(1))) uint64_t GU64;
  __shared__ int sh_err;
  __shared__ int64_t sh_n;
  const unsigned g = blockIdx.x;
  int c = 0, hi = t.n;  // the segment whose tiles hold block g: tile0[c] <= g < tile0[c + 1]
  while (hi - c > 1) {
    const int mid = (c + hi) >> 1;
    if (t.tile0[mid] <= g) c = mid;
    else hi = mid;
  }
  const WireSeg a = t.seg[c];  // scalar loads from the kernel argument: a copy, so the table is never spilled
  const uint32_t x = g - t.tile0[c];
  if (a.unpack) {  // uniform per workgroup
    if (threadIdx.x == 0) {  // the header, before any payload byte is loaded
      const uint64_t hd = *(const GU64*)a.hdr;
      int64_t n = 0;
      const int err = wire_check_header(a, hd, &n);
      sh_err = err;
      sh_n = n;
      if (x == 0) *(GU64*)a.slot = wire_slot_word(err, n);
    }
    __syncthreads();
    if (sh_err) return;
    wire_arms<true, NT>(a, x, sh_n);
  } else {
    if (x == 0 && threadIdx.x == 0) *(GU64*)a.hdr = a.header;  // one 8-byte store
    wire_arms<false, NT>(a, x, 0);
  }
}

static_assert(WireTile<false>::gran == kStridedTile && WireTile<true>::gran == kStridedTileNT,
              "the tiles are the strided moves'");

// MPJX_STRIDED_NT_MIN_MIB (read per call) moves the streaming threshold, as for k_pack
static int64_t wire_stream_bytes() {
  const char* e = getenv("MPJX_STRIDED_NT_MIN_MIB");
  const long m = e ? atol(e) : 0;
  return m > 0 ? (int64_t)m << 20 : kStridedStreamBytes;
}

hipError_t launch_wire(const std::vector<WireSeg>& segs, hipStream_t s, int64_t* launches) {
  if (segs.empty()) return hipSuccess;
  int64_t total = 0;
  for (const WireSeg& a : segs) {
    if (a.glog < a.wlog || a.glog > 4 || a.wlog > 3) return hipErrorInvalidValue;
    total += (int64_t)a.ngran << a.glog;
  }
  const bool nt = total >= wire_stream_bytes();
  std::vector<WireTable> tabs;
  plan_wire_tables(segs, nt ? kStridedTileNT : kStridedTile, &tabs);
  for (const WireTable& t : tabs) {
    const unsigned grid = t.tile0[t.n];
    if (nt) hipLaunchKernelGGL((k_wire<true>), dim3(grid), dim3(WireTile<true>::TH), 0, s, t);
    else hipLaunchKernelGGL((k_wire<false>), dim3(grid), dim3(WireTile<false>::TH), 0, s, t);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (launches) ++*launches;
  }
  return hipSuccess;
}

}  // namespace mpjx
