// mpjx_k_msgs_pool.hip — k_msgs_pool: a batch of matched pairs of PERSISTENT requests in one launch, their
// segments read from the communicator's device pool (mpjx_msgs_pool_plan.hpp) instead of the kernel argument.
//   - k_msgs carries its segments in a 4-KiB argument: kMsgsMax = 24 per launch. A pair of two persistent
//     requests has the same segment at every start, so it is stored once (k_msgs_pool_put) and a launch carries
//     only MsgsIndex: up to kPoolBatchMax = 512 slot numbers and the prefix of their tiles.
//   - Block g searches tile0[] for its entry c, as k_msgs does, and reads its segment from pool[slot[c]]. The
//     address is uniform per workgroup, so the segment is fetched once per wave and the branch on its kind stays
//     scalar.
//   - The per-lane code is k_msgs' own (mpjx_k_msgs_tile.hpp): bytes kind and granule kind, both tile shapes.
//   - k_msgs_pool_put stores up to kPoolPutMax segments from its argument into their slots, word by word with
//     ordinary vector stores: no host staging buffer has to outlive the call. It runs on the communicator's
//     stream, after every launch that read the slots it overwrites and before every launch that reads them.
// The several-device form (a pool on one device, operands on another) has no machine to be run on and is
// unverified, as k_msgs' is.
#include "mpjx_k_msgs_tile.hpp"
#include "mpjx_msgs_pool_plan.hpp"

namespace mpjx {

template <bool NT>
__global__ __launch_bounds__(MsgsTile<NT>::TH) void k_msgs_pool(const MsgSeg* __restrict__ pool, MsgsIndex ix) {
  const unsigned g = blockIdx.x;
  int c = 0, hi = ix.n;  // the entry whose tiles hold block g: tile0[c] <= g < tile0[c + 1]
  while (hi - c > 1) {
    const int mid = (c + hi) >> 1;
    if (ix.tile0[mid] <= g) c = mid;
    else hi = mid;
  }
  msgs_tile<NT>(pool[ix.slot[c]], g - ix.tile0[c], ix.tile0[c + 1] - ix.tile0[c]);
}

constexpr int kPutWords = (int)(sizeof(MsgSeg) / sizeof(uint32_t));

// Block b stores entry b: one word per lane
__global__ __launch_bounds__(64) void k_msgs_pool_put(MsgSeg* pool, PoolPut p) {
  const int b = (int)blockIdx.x;
  if (b >= p.n) return;
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&p.seg[b]);
  uint32_t* dst = reinterpret_cast<uint32_t*>(&pool[p.slot[b]]);
  for (int w = (int)threadIdx.x; w < kPutWords; w += 64) dst[w] = src[w];
}

hipError_t launch_msgs_pool(const MsgSeg* pool, const std::vector<PoolRef>& refs, bool nt, hipStream_t s,
                            int64_t* launches) {
  if (refs.empty()) return hipSuccess;
  for (const PoolRef& r : refs)
    if (r.slot >= kPoolSlots || r.tiles == 0) return hipErrorInvalidValue;
  std::vector<MsgsIndex> ixs;
  plan_msgs_indices(refs, &ixs);
  for (const MsgsIndex& ix : ixs) {
    const unsigned grid = ix.tile0[ix.n];
    if (nt) hipLaunchKernelGGL((k_msgs_pool<true>), dim3(grid), dim3(MsgsTile<true>::TH), 0, s, pool, ix);
    else hipLaunchKernelGGL((k_msgs_pool<false>), dim3(grid), dim3(MsgsTile<false>::TH), 0, s, pool, ix);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (launches) ++*launches;
  }
  return hipSuccess;
}

hipError_t launch_msgs_pool_put(MsgSeg* pool, const std::vector<std::pair<MsgSeg, int>>& puts, hipStream_t s) {
  for (size_t at = 0; at < puts.size(); at += kPoolPutMax) {
    PoolPut p;
    for (size_t i = at; i < puts.size() && p.n < kPoolPutMax; i++) {
      if (puts[i].second < 0 || puts[i].second >= kPoolSlots) return hipErrorInvalidValue;
      p.seg[p.n] = puts[i].first;
      p.slot[p.n] = (uint16_t)puts[i].second;
      p.n++;
    }
    hipLaunchKernelGGL(k_msgs_pool_put, dim3((unsigned)p.n), dim3(64), 0, s, pool, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace mpjx
