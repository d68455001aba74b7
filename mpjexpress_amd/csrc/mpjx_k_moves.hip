// mpjx_k_moves.hip — k_moves: up to kMoveMax independent block moves (src, dst, bytes) in one launch,
// for the block-move collectives (Allgather(v), Gatherv, Scatterv, Alltoall(v)), whose displacements are
// in elements: any (src mod 16, dst mod 16) pair, ragged lengths, empty segments.
//   - The grid is the SUM of the segments' tiles (MoveTable::tile0, a prefix sum planned on the host,
//     mpjx_moves_plan.hpp): block g searches the prefix for its (segment, tile). k_copies' grid is
//     (tiles of the longest copy) x (copies), mostly empty blocks when the lengths differ.
//   - Tiles lie on the DESTINATION's 16-B grid: every whole vector is one aligned 16-B store. The head
//     (up to the destination's alignment) and the tail (past the last whole vector) are byte stores by
//     the first and the last tile of the segment, inside [dst, dst + bytes) only.
//   - The source of a whole vector starts `sh` bytes into an aligned 16-B granule, sh uniform per
//     segment: sh = 0 is one aligned 16-B load, otherwise two aligned 16-B loads (both granules hold
//     at least one byte of the segment, so neither load leaves the pages the segment touches) combined
//     by a dword select on sh / 4 and v_alignbyte_b32 on sh % 4. k_copies moves such pairs one byte per
//     lane per instruction.
// Tile shapes and the streaming threshold are k_copies' (mpjx_k_util.hip): 256 lanes x 4 vectors with
// the default cache policy; from 64 MiB per call 512 lanes x 1 vector, non-temporal loads and stores,
// chosen there on cold buffers (profiles/r02/cold/tune_cold_sweep2.txt: 83.3 us per 256 MiB).
#include "mpjx_kernels.hpp"

namespace mpjx {

template <bool NT>
struct MoveTile {
  static constexpr int TH = NT ? 512 : 256;
  static constexpr int U = NT ? 1 : 4;
  static constexpr int64_t vecs = TH * U;
};

// MoveSeg carries addresses as integers (the planner's header has no HIP types); loads and stores through
// pointers cast from them would be FLAT instructions. Every segment is device-accessible global memory, so
// the kernel says so: global_load / global_store, as k_copies gets from its typed kernel-argument pointers.
using gv4u = __attribute__((address_space(1))) v4u;
using gu8 = __attribute__((address_space(1))) unsigned char;

template <bool NT>
__device__ __forceinline__ v4u ldg(const gv4u* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT>
__device__ __forceinline__ void stg(gv4u* p, v4u v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// The 16 bytes that start sh bytes (1..15, uniform) into the 32 bytes {lo, hi}
__device__ __forceinline__ v4u shift_bytes(v4u lo, v4u hi, unsigned sh) {
  const unsigned w[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  const unsigned q = sh >> 2, b = sh & 3u;
  unsigned x[5];
#pragma unroll
  for (int k = 0; k < 5; k++) x[k] = q == 0 ? w[k] : q == 1 ? w[k + 1] : q == 2 ? w[k + 2] : w[k + 3];
  v4u r;
#pragma unroll
  for (int k = 0; k < 4; k++) r[k] = __builtin_amdgcn_alignbyte(x[k + 1], x[k], b);  // ({hi, lo} >> 8 b)
  return r;
}

// ONE: a table of one segment (every P = 1 call, and the rank's own block on the exchange engines) skips
// the search, so the block's first vector load waits for one round of kernel-argument loads instead of two
// (the segment count, then the segment), as k_copies' does. 256 MiB aligned and cold (profiles/moves/):
// 92.2 us with the search and flat accesses, 90.7 without the search, 86.6 with global accesses as well,
// against 86.5-87.1 for k_copies in the same runs.
template <bool NT, bool ONE>
__global__ __launch_bounds__(MoveTile<NT>::TH) void k_moves(MoveTable t) {
  constexpr int TH = MoveTile<NT>::TH;
  constexpr int U = MoveTile<NT>::U;
  constexpr int64_t VECS = MoveTile<NT>::vecs;
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
  const MoveSeg sg = t.seg[c];
  const unsigned first = ONE ? 0u : t.tile0[c];  // tile0[0] = 0
  const int64_t x = g - first, last = (int64_t)(t.tile0[c + 1] - first) - 1;
  const MoveGeom gm = move_geom(sg.dst, sg.bytes);
  int64_t v0, v1;
  move_tile_vectors(gm, x, VECS, &v0, &v1);
  // vector i of the segment: the aligned 16 B at d4 + i, from the 16 B at s0 + 16 i
  gv4u* d4 = (gv4u*)(sg.dst - gm.da);
  const uint64_t s0 = sg.src - gm.da;
  const unsigned sh = (unsigned)(s0 & 15u);
  const gv4u* s4 = (const gv4u*)(s0 - sh);
  const int64_t base = x * VECS;
  if (sh == 0) {
    v4u v[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = base + u * TH + threadIdx.x;
      if (i >= v0 && i < v1) v[u] = ldg<NT>(s4 + i);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = base + u * TH + threadIdx.x;
      if (i >= v0 && i < v1) stg<NT>(d4 + i, v[u]);
    }
  } else {
    v4u a[U], b[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = base + u * TH + threadIdx.x;
      if (i >= v0 && i < v1) {
        a[u] = ldg<NT>(s4 + i);
        b[u] = ldg<NT>(s4 + i + 1);
      }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int64_t i = base + u * TH + threadIdx.x;
      if (i >= v0 && i < v1) stg<NT>(d4 + i, shift_bytes(a[u], b[u], sh));
    }
  }
  const gu8* S = (const gu8*)sg.src;
  gu8* D = (gu8*)sg.dst;
  if (x == 0)
    for (int64_t k = threadIdx.x; k < gm.head; k += TH) D[k] = S[k];
  if (x == last)
    for (int64_t k = gm.ts + threadIdx.x; k < sg.bytes; k += TH) D[k] = S[k];
}

hipError_t launch_moves(const MoveList& l, hipStream_t s) {
  int64_t total = 0;
  for (const MoveSeg& m : l.segs) total += m.bytes > 0 ? m.bytes : 0;
  if (total == 0) return hipSuccess;
  const bool nt = total >= ((int64_t)64 << 20);
  std::vector<MoveTable> tabs;
  plan_tables(l.segs, nt ? MoveTile<true>::vecs : MoveTile<false>::vecs, &tabs);
  for (const MoveTable& t : tabs) {
    const unsigned grid = t.tile0[t.n];
    if (nt && t.n == 1) hipLaunchKernelGGL((k_moves<true, true>), dim3(grid), dim3(MoveTile<true>::TH), 0, s, t);
    else if (nt) hipLaunchKernelGGL((k_moves<true, false>), dim3(grid), dim3(MoveTile<true>::TH), 0, s, t);
    else if (t.n == 1) hipLaunchKernelGGL((k_moves<false, true>), dim3(grid), dim3(MoveTile<false>::TH), 0, s, t);
    else hipLaunchKernelGGL((k_moves<false, false>), dim3(grid), dim3(MoveTile<false>::TH), 0, s, t);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace mpjx
