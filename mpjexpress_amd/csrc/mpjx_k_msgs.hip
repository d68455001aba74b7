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
// The per-lane code is mpjx_k_msgs_tile.hpp's, shared with k_msgs_pool (mpjx_k_msgs_pool.hip).
// Tile shapes are the other move kernels': 256 lanes x 4 with the default cache policy, 512 lanes x 1 with
// non-temporal loads and stores from kStridedStreamBytes of batch payload (a threshold taken over from
// k_strided, not measured on this kernel).
#include "mpjx_k_msgs_tile.hpp"

namespace mpjx {

template <bool NT>
__global__ __launch_bounds__(MsgsTile<NT>::TH) void k_msgs(MsgsTable t) {
  const unsigned g = blockIdx.x;
  int c = 0, hi = t.n;  // the segment whose tiles hold block g: tile0[c] <= g < tile0[c + 1]
  while (hi - c > 1) {
    const int mid = (c + hi) >> 1;
    if (t.tile0[mid] <= g) c = mid;
    else hi = mid;
  }
  msgs_tile<NT>(t.seg[c], g - t.tile0[c], t.tile0[c + 1] - t.tile0[c]);
}

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
