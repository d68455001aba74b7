// mpjx_msgs_pool_plan.hpp — the device segment pool of the persistent requests and the launch index of
// k_msgs_pool (mpjx_k_msgs_pool.hip). No HIP include: plain C++17, compiled, tested and sanitized on the CPU
// (tests/cpp/msgs_pool_plan_test.cpp, tests/cpp/preq_plan_test.cpp); the kernel includes the same header.
//
// A pair of two persistent requests has the same addresses, layouts and length at every start, so its MsgSeg
// (mpjx_msgs_plan.hpp) is planned once and kept in a slot of a device array the communicator owns. A launch then
// carries no segments, only an index: the slots of the batch and the prefix of their tiles. Any subset of a
// rank's pairs can be a batch, so the index is made per launch and nothing about a batch is kept.
//   PoolMap     host side: (send serial, recv serial) -> slot, with the segment's tile counts for both tile sizes.
//               Serials are never reused, so the entry of a freed request is never looked up again; its slot is
//               reclaimed when a put finds no free slot. Not thread-safe: the owning rank's thread calls it.
//   PoolPut     the argument of the put kernel: up to kPoolPutMax (segment, slot) entries.
//   MsgsIndex   the argument of k_msgs_pool: up to kPoolBatchMax slots and tile0[], as MsgsTable's.
#pragma once
#include <atomic>
#include <memory>
#include <unordered_map>

#include "mpjx_msgs_plan.hpp"

namespace mpjx {

constexpr int kPoolSlots = 1024;     // segments a communicator keeps on the device (fits uint16_t)
constexpr int kPoolBatchMax = 512;   // segments per k_msgs_pool launch
constexpr int kPoolPutMax = kMsgsMax;  // segments per put launch

struct MsgsIndex {
  uint32_t tile0[kPoolBatchMax + 1];  // tile0[c] = first block of entry c; tile0[n] = the grid
  uint16_t slot[kPoolBatchMax];
  int n = 0;
};
static_assert(sizeof(MsgsIndex) < 4096, "the index is a kernel argument");

struct PoolPut {
  MsgSeg seg[kPoolPutMax];
  uint16_t slot[kPoolPutMax];
  int n = 0;
};
static_assert(sizeof(PoolPut) <= 4096 - 8, "the put list and the pool's address are kernel arguments");
static_assert(sizeof(MsgSeg) % 4 == 0, "the put kernel stores a segment word by word");

// One pooled pair of a batch: its slot and its tiles for the tile size of the launch
struct PoolRef {
  uint16_t slot;
  uint32_t tiles;
};

// The launch indices of `refs`, in order: an index is closed when it holds kPoolBatchMax entries or max_tiles
// tiles. Every entry has at least one tile and at most max_tiles (PoolMap::put refuses others). Every index has
// n >= 1 and tile0[n] >= 1.
inline void plan_msgs_indices(const std::vector<PoolRef>& refs, std::vector<MsgsIndex>* out,
                              int64_t max_tiles = kMoveMaxTiles, int batch_max = kPoolBatchMax) {
  out->clear();
  MsgsIndex ix;
  ix.tile0[0] = 0;
  for (const PoolRef& r : refs) {
    if (ix.n == batch_max || (int64_t)ix.tile0[ix.n] + (int64_t)r.tiles > max_tiles) {
      if (ix.n > 0) out->push_back(ix);
      ix.n = 0;
    }
    ix.slot[ix.n] = r.slot;
    ix.tile0[ix.n + 1] = ix.tile0[ix.n] + r.tiles;
    ix.n++;
  }
  if (ix.n > 0) out->push_back(ix);
}

class PoolMap {
 public:
  struct Entry {
    uint16_t slot;
    uint32_t tiles, tiles_nt;  // msg_tiles for kStridedTile and kStridedTileNT
    int64_t bytes;
    std::shared_ptr<std::atomic<bool>> sfreed, rfreed;  // the two requests' flags (Persist)
  };
  explicit PoolMap(int slots = kPoolSlots) : cap_(slots) {
    for (int i = slots - 1; i >= 0; i--) free_.push_back((uint16_t)i);
  }
  int capacity() const { return cap_; }
  int in_use() const { return cap_ - (int)free_.size(); }

  const Entry* find(uint64_t ss, uint64_t rs) const {
    auto it = map_.find(Key{ss, rs});
    return it == map_.end() ? nullptr : &it->second;
  }

  // True if `m` can be pooled at all: a nonempty segment of at most max_tiles tiles in both tile sizes
  static bool poolable(const MsgSeg& m, int64_t max_tiles = kMoveMaxTiles) {
    return m.bytes > 0 && msg_tiles(m, kStridedTile) <= max_tiles && msg_tiles(m, kStridedTileNT) <= max_tiles;
  }

  // A slot for the pair (ss, rs) whose segment is m, or -1 when the pool is full of live pairs. With no free
  // slot, the slots of pairs one of whose requests was freed are reclaimed first.
  int put(uint64_t ss, uint64_t rs, const MsgSeg& m, const std::shared_ptr<std::atomic<bool>>& sfreed,
          const std::shared_ptr<std::atomic<bool>>& rfreed, int64_t max_tiles = kMoveMaxTiles) {
    if (!poolable(m, max_tiles) || map_.count(Key{ss, rs})) return -1;
    if (free_.empty()) reclaim();
    if (free_.empty()) return -1;
    Entry e;
    e.slot = free_.back();
    free_.pop_back();
    e.tiles = (uint32_t)msg_tiles(m, kStridedTile);
    e.tiles_nt = (uint32_t)msg_tiles(m, kStridedTileNT);
    e.bytes = m.bytes;
    e.sfreed = sfreed;
    e.rfreed = rfreed;
    map_.emplace(Key{ss, rs}, e);
    return e.slot;
  }

  // The pair leaves the map and its slot is free again (a put whose store could not be enqueued)
  void erase(uint64_t ss, uint64_t rs) {
    auto it = map_.find(Key{ss, rs});
    if (it == map_.end()) return;
    free_.push_back(it->second.slot);
    map_.erase(it);
  }

  // Frees the slots of dead pairs; returns how many
  int reclaim() {
    int n = 0;
    for (auto it = map_.begin(); it != map_.end();) {
      const Entry& e = it->second;
      if ((e.sfreed && e.sfreed->load(std::memory_order_acquire)) || (e.rfreed && e.rfreed->load(std::memory_order_acquire))) {
        free_.push_back(e.slot);
        it = map_.erase(it);
        n++;
      } else {
        ++it;
      }
    }
    return n;
  }

 private:
  struct Key {
    uint64_t s, r;
    bool operator==(const Key& o) const { return s == o.s && r == o.r; }
  };
  struct Hash {
    size_t operator()(const Key& k) const { return (size_t)(k.s * 0x9E3779B97F4A7C15ull ^ (k.r + (k.s << 32))); }
  };
  std::unordered_map<Key, Entry, Hash> map_;
  std::vector<uint16_t> free_;
  int cap_;
};

}  // namespace mpjx
