// mpjx_k_pack.hip — k_pack: one mpjbuf section written from, or read into, a buffer laid out by any datatype
// (mpjx_pack / mpjx_unpack; the section format and the granule: mpjx_pack_plan.hpp). Layout, byte swap and header
// in ONE HBM pass: a caller without it moves the layout into scratch (k_strided / k_indexed), swaps the scratch
// in a second pass and writes the header from the host.
//   - Shaped like k_indexed / k_strided (see there for the tiles and the cache policies): one lane moves one
//     granule of the packed stream, neighbouring lanes take neighbouring granules. The buffer-side address of
//     granule q is strided_addr's or indexed_addr's (the LDS copy of a table of up to kPackLdsBlocks blocks, the
//     direct search above that, as k_indexed chooses), or linear for a contiguous layout; the payload-side
//     address is pay + q * granule. The granule holds whole base words (never less than one: the planner
//     asserts it), which are byte-swapped in registers between the load and the store: words of 1 (no swap), 2,
//     4 or 8 bytes; a pair type swaps its base word.
//   - UNPACK selects the direction. Pack: lane 0 of block 0 stores the 8 header bytes with one 8-byte store.
//     Unpack: lane 0 of EVERY block loads the 8 header bytes (L2-resident after the first block) and checks
//     them before any payload byte is read: a wrong type code (MPJX_MPJBUF_BAD_TYPE), a count that is negative
//     or whose payload passes the end of the image (_OVERRUN), a count other than the expected one (_BAD_COUNT),
//     in k_mpjbuf's order. A bad header ends every block before its first payload load, leaves the buffer
//     untouched, and block 0 stores the code into *status. The host has already checked that the EXPECTED
//     payload lies inside the image, so a header that passes covers every load.
//   - Only bytes inside the layout's blocks are stored by an unpack; gaps keep their contents.
// Loads and stores go through global-address-space pointers. 256 lanes x 4 granules with the default cache
// policy; from the streaming threshold of the strided moves (64 MiB of payload, MPJX_STRIDED_NT_MIN_MIB) 512
// lanes x 1 granule, non-temporal.
#include <stdlib.h>

#include "mpjx_kernels.hpp"
#include "mpjx_pack_plan.hpp"

namespace mpjx {

namespace {

constexpr int kPackLdsBlocks = 512;  // entries the LDS form can hold (k_indexed's per side): 8 KiB per workgroup

template <bool NT>
struct PackTile {
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

// `lds`: the workgroup's copy of the layout's table, or nullptr to search the device table
template <int GLOG>
__device__ __forceinline__ uint64_t lay_addr(const PackSeg& a, const IdxEnt* lds, uint32_t q) {
  if (a.lin) return a.lay.r.base + ((uint64_t)q << GLOG);  // uniform
  if (a.lay.tab && lds) {
    typedef __attribute__((address_space(3))) const IdxEnt LE;  // ds_read, not a flat load
    LE* p = (LE*)lds;
    return irregular_addr(a.lay, q, GLOG, [p](uint32_t i) { return IdxEnt{p[i].off, p[i].pre}; });
  }
  return indexed_addr(a.lay, q, GLOG);
}

template <bool UNPACK, bool NT, int GLOG, int WS>
__device__ __forceinline__ void pack_tile(const PackSeg& a, uint32_t x, const IdxEnt* lds) {
  static_assert((1 << GLOG) >= WS, "a granule holds whole base words");
  constexpr int TH = PackTile<NT>::TH;
  constexpr int U = PackTile<NT>::U;
  using T = typename Granule<GLOG>::type;
  using GT = __attribute__((address_space(1))) T;
  // ngran < 2^31: q0 + u * TH + t stays far below 2^32; computed in 64 bits as the other move kernels do
  const uint64_t q0 = (uint64_t)x * (TH * U) + threadIdx.x;
  T v[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const uint64_t q = q0 + (uint64_t)u * TH;
    if (q < a.ngran) {
      const GT* p = (const GT*)(UNPACK ? a.pay + (q << GLOG) : lay_addr<GLOG>(a, lds, (uint32_t)q));
      if constexpr (NT) v[u] = __builtin_nontemporal_load(p);
      else v[u] = *p;
    }
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    const uint64_t q = q0 + (uint64_t)u * TH;
    if (q < a.ngran) {
      const T w = swap_words<WS>(v[u]);
      GT* p = (GT*)(UNPACK ? lay_addr<GLOG>(a, lds, (uint32_t)q) : a.pay + (q << GLOG));
      if constexpr (NT) __builtin_nontemporal_store(w, p);
      else *p = w;
    }
  }
}

}  // namespace

template <bool UNPACK, bool NT, bool LDS>
__global__ __launch_bounds__(PackTile<NT>::TH) void k_pack(PackSeg a, uint32_t cap) {
  typedef __attribute__((address_space(1))) uint64_t GU64;
  constexpr int TH = PackTile<NT>::TH;
  __shared__ int bad;
  const IdxEnt* lds = nullptr;
  if constexpr (LDS) {
    __shared__ IdxEnt tab[kPackLdsBlocks];
    if (a.lay.tab && a.lay.r.nb.d <= cap) {  // cap <= kPackLdsBlocks
      for (uint32_t i = threadIdx.x; i < a.lay.r.nb.d; i += TH) tab[i] = idx_entry(a.lay.tab, i);
      lds = tab;
    }
  }
  if constexpr (UNPACK) {
    if (threadIdx.x == 0) {  // the header, before any payload byte is read
      const uint64_t hd = *(const GU64*)a.hdr;
      const int64_t n = (int64_t)(int32_t)__builtin_bswap32((uint32_t)(hd >> 32));
      int err = 0;
      if ((int)(hd & 0xffu) != a.code) err = 1;                // MPJX_MPJBUF_BAD_TYPE
      else if (n < 0 || (n << a.wlog) > a.room) err = 3;       // MPJX_MPJBUF_OVERRUN
      else if (n != a.words) err = 2;                          // MPJX_MPJBUF_BAD_COUNT
      bad = err;
      if (err && blockIdx.x == 0) *a.status = err;
    }
  }
  if constexpr (UNPACK || LDS) __syncthreads();
  if constexpr (UNPACK) {
    if (bad) return;
  } else {
    if (blockIdx.x == 0 && threadIdx.x == 0) *(GU64*)a.hdr = a.header;  // one 8-byte store
  }
  const uint32_t x = blockIdx.x;
#define MPJX_PK(G, W)                               \
  case (G) * 4 + (W):                               \
    pack_tile<UNPACK, NT, G, (1 << (W))>(a, x, lds); \
    break;
  switch (a.glog * 4 + a.wlog) {  // uniform per launch; the planner keeps glog >= wlog
    MPJX_PK(0, 0) MPJX_PK(1, 0) MPJX_PK(2, 0) MPJX_PK(3, 0) MPJX_PK(4, 0)
    MPJX_PK(1, 1) MPJX_PK(2, 1) MPJX_PK(3, 1) MPJX_PK(4, 1)
    MPJX_PK(2, 2) MPJX_PK(3, 2) MPJX_PK(4, 2)
    MPJX_PK(3, 3) MPJX_PK(4, 3)
    default: break;
  }
#undef MPJX_PK
}

static_assert(PackTile<false>::gran == kStridedTile && PackTile<true>::gran == kStridedTileNT,
              "the tiles are the strided moves'");

// MPJX_STRIDED_NT_MIN_MIB (read per call) moves the streaming threshold, as for k_strided and k_indexed
static int64_t stream_bytes() {
  const char* e = getenv("MPJX_STRIDED_NT_MIN_MIB");
  const long m = e ? atol(e) : 0;
  return m > 0 ? (int64_t)m << 20 : kStridedStreamBytes;
}

// MPJX_INDEXED_LDS_MAX_BLOCKS (read per call), as for k_indexed: the largest table searched in LDS
static uint32_t lds_max_blocks() {
  const char* e = getenv("MPJX_INDEXED_LDS_MAX_BLOCKS");
  const long m = e ? atol(e) : kPackLdsBlocks;
  return (uint32_t)std::min<long>(std::max<long>(m, 0), kPackLdsBlocks);
}

template <bool UNPACK, bool NT>
static void launch_form(const PackSeg& a, bool lds, uint32_t cap, hipStream_t s) {
  const int64_t tiles = strided_tiles(a.ngran, PackTile<NT>::gran);
  const unsigned grid = (unsigned)std::max<int64_t>(tiles, 1);  // a header-only section still runs block 0
  if (lds) hipLaunchKernelGGL((k_pack<UNPACK, NT, true>), dim3(grid), dim3(PackTile<NT>::TH), 0, s, a, cap);
  else hipLaunchKernelGGL((k_pack<UNPACK, NT, false>), dim3(grid), dim3(PackTile<NT>::TH), 0, s, a, cap);
}

hipError_t launch_pack(const PackSeg& a, bool unpack, hipStream_t s) {
  if (a.glog < a.wlog || a.glog > 4 || a.wlog > 3) return hipErrorInvalidValue;
  const bool nt = ((int64_t)a.ngran << a.glog) >= stream_bytes();
  const uint32_t cap = lds_max_blocks();
  const bool lds = a.ngran > 0 && !a.lin && a.lay.tab && a.lay.r.nb.d <= cap;
  if (unpack && nt) launch_form<true, true>(a, lds, cap, s);
  else if (unpack) launch_form<true, false>(a, lds, cap, s);
  else if (nt) launch_form<false, true>(a, lds, cap, s);
  else launch_form<false, false>(a, lds, cap, s);
  return hipGetLastError();
}

}  // namespace mpjx
