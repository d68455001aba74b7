// mpjx_p2p_plan.hpp — the matching engine of the point-to-point calls (Send, Recv, Isend, Irecv, Sendrecv,
// Waitall: src/mpi/Comm.java:381-2460, src/mpi/Request.java) and the first-fit allocator of the eager slab. No
// HIP include: plain C++17, compiled, tested and sanitized on the CPU (tests/cpp/p2p_match_test.cpp); the
// library's entry points (mpjx_p2p.hip) drive exactly this code.
//
// One Mailbox per multicore world, with its own mutex and condition variable: point-to-point and collective
// traffic never meet (the reference's two contexts), and a sub-communicator, being a world of its own, has a
// mailbox of its own. Per destination rank the mailbox keeps two lists in post order: posted receives and
// unmatched sends. The matching rule is MPI's: a send (src, dst, tag) matches the first posted receive at dst
// whose source is src or ANY_SOURCE and whose tag is tag or ANY_TAG; a receive matches the first unmatched
// send likewise. Both lists are walked front to back, which gives non-overtaking per (src, dst).
//
// A matched pair goes MATCHED -> CLAIMED -> LAUNCHED. Nothing is launched at post time: a call that waits
// claims EVERY matched, unclaimed pair its rank is a party to (claim), moves the batch on its own stream and
// marks it LAUNCHED with the batch's completion event (launched). Either party may move a pair, so no legal
// order of waits deadlocks. The base-type test passes when either side is MPI.PACKED (kP2PPacked): such a pair is
// marked for k_wire (PairWire) and checked for what the host can know of it. Mailbox::peek / probe are Probe and
// Iprobe: they look at the unmatched sends and consume nothing.
// A pair that fails its checks at match time (base types differ, the message is
// longer than the receive layout, a self-message whose layouts share a byte) is FAILED at once on both
// requests; nothing moves and the world stays usable.
#pragma once
#include <stdint.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "mpjx_strided_plan.hpp"

namespace mpjx {

constexpr int kAnySource = -2, kAnyTag = -2, kProcNull = -3;  // src/mpi/MPI.java:132-136
constexpr int kUndefined = -1;
constexpr int kP2POk = 0, kP2PErrArg = -1, kP2PErrInternal = -7;  // MPJX_SUCCESS / _ERR_ARG / _ERR_INTERNAL
constexpr int kP2PPacked = 9;  // MPI.PACKED's base type code: the request's buffer is an mpjbuf image, its word 1 byte
// A pair with PACKED on exactly one side is moved by k_wire (mpjx_wire_plan.hpp): packed on the fly into the
// receiver's image (typed -> PACKED) or unpacked on the fly from the sender's (PACKED -> typed)
enum PairWire { kPairPlain = 0, kPairPack = 1, kPairUnpack = 2 };

enum PairState { kPairMatched = 0, kPairClaimed = 1, kPairLaunched = 2, kPairFailed = 3 };

struct P2PPair;

// One posted send or receive. `peer` is the destination of a send and the source (or ANY_SOURCE) asked for
// by a receive; `lay` the layout in bytes (absolute addresses), `bytes` its packed bytes: the message's
// length for a send, the room for a receive.
struct P2PReq {
  bool send = false;
  int rank = 0, peer = 0, tag = 0;
  int base = 0, bsz = 1;
  int64_t bytes = 0;
  int64_t count = 0;   // the receive count (items), for the status of a receive whose type has size 0
  bool empty_type = false;
  SideBytes lay;
  std::shared_ptr<void> ready;  // the poster's ready event, or none when its stream was idle at post
  std::shared_ptr<P2PPair> pair;
  bool null_peer = false;  // PROC_NULL: complete at once
  bool orphan = false;     // its communicator was destroyed, or its wait gave up: no longer in any list
  bool eager = false;      // an eager send: its message lies in the sender's slab and nobody waits for it
  bool consumed = false;   // eager: the receiver has completed its wait, the slab chunk may be reused
  // An activation of a persistent request (Persist below): the serial of the request behind it, and that
  // request's `freed` flag. A plain request carries 0 and none.
  uint64_t serial = 0;
  std::shared_ptr<std::atomic<bool>> freed;
  std::string envelope() const {
    return std::string(send ? "send" : "recv") + "(rank " + std::to_string(rank) + (send ? " -> " : " <- ") +
           (peer == kAnySource ? std::string("ANY_SOURCE") : std::to_string(peer)) + ", tag " +
           (tag == kAnyTag ? std::string("ANY_TAG") : std::to_string(tag)) + ", " + std::to_string(bytes) + " B)";
  }
};

struct P2PPair {
  std::shared_ptr<P2PReq> s, r;
  int state = kPairMatched;
  int mover = -1;               // the rank that claimed it
  std::shared_ptr<void> done;   // the completion event of the batch that moved it (kept alive by the pair)
  int err = kP2POk;
  std::string msg;
  int wire = kPairPlain;
  // kPairUnpack: the 8-byte host-readable slot {int32 code, int32 n} the kernel stores, alive as long as the
  // pair; `resolved` once a party has read it after the batch's completion event passed, n then in wire_n
  std::shared_ptr<void> slot;
  bool resolved = false;
  int64_t wire_n = 0;
};

// What a completed request reports (mpjx_status)
struct P2PStatus {
  int source = kProcNull, tag = kAnyTag, error = kP2POk;
  int64_t elements = 0, bytes = 0;
};

inline P2PStatus p2p_status(const P2PReq& q) {
  P2PStatus st;
  if (q.null_peer || !q.pair) return st;
  const P2PPair& p = *q.pair;
  st.error = p.err;
  if (q.send && q.serial != 0) return st;  // Prequest: only the receivers have status values (the empty status)
  st.source = p.s->rank;
  st.tag = p.s->tag;
  if (p.err != kP2POk) return st;
  st.bytes = p.s->bytes;
  st.elements = p.s->bytes / (q.bsz > 0 ? q.bsz : 1);
  if (!q.send && p.wire == kPairPack) st.bytes = st.elements = 8 + p.s->bytes;  // the section: header and payload
  if (!q.send && p.wire == kPairUnpack) {  // what the header announced, from the slot
    st.elements = p.wire_n;
    st.bytes = p.wire_n * q.bsz;
  }
  if (!q.send && q.empty_type) st.elements = q.count;  // Comm.java:1526-1531: a type of size 0 reports the count
  return st;
}

// count and elements of `st` for a type of `size` base elements per item (Comm.java:1517-1531)
inline void p2p_get_count(int64_t st_elements, int64_t size, int64_t* count, int64_t* elements) {
  if (size != 0) {
    *elements = st_elements;
    *count = st_elements % size == 0 ? st_elements / size : kUndefined;
  } else {
    *count = st_elements;
    *elements = kUndefined;
  }
}

class Mailbox {
 public:
  using Clock = std::chrono::steady_clock;
  explicit Mailbox(int P) : recvs_((size_t)P), sends_((size_t)P), P_(P) {}
  int size() const { return P_; }

  // Read once at world creation (mpjx_p2p.hip): MPJX_P2P_TIMEOUT_S, MPJX_P2P_EAGER_KIB, MPJX_P2P_EAGER_POOL_MIB,
  // MPJX_P2P_BATCH, MPJX_P2P_POOL
  double timeout_s = 300;
  int64_t eager_bytes = (int64_t)128 << 10;
  int64_t pool_bytes = (int64_t)8 << 20;
  bool batch = true;
  bool seg_pool = true;  // MPJX_P2P_POOL: pairs of two persistent requests keep their segment on the device

  // Posts q (send: to q->peer; receive: at q->rank) and matches it if a partner waits. A PROC_NULL peer
  // completes at once. Returns the pair when one was made (FAILED pairs included).
  std::shared_ptr<P2PPair> post(const std::shared_ptr<P2PReq>& q) {
    std::shared_ptr<P2PPair> made;
    bool wake;
    {
      std::lock_guard<std::mutex> g(mu_);
      made = post_locked(q);
      wake = made || probers_ > 0;  // a probe sleeps for an unmatched send too
    }
    if (wake) cv_.notify_all();
    return made;
  }

  // Posts every request of `qs` under ONE acquisition of the lock, in array order: the order non-overtaking
  // sees (Prequest.Startall). Returns the pairs made.
  size_t post_all(const std::vector<std::shared_ptr<P2PReq>>& qs) {
    size_t made = 0;
    bool wake;
    {
      std::lock_guard<std::mutex> g(mu_);
      for (const auto& q : qs) made += post_locked(q) ? 1 : 0;
      wake = made > 0 || probers_ > 0;
    }
    if (wake) cv_.notify_all();
    return made;
  }

  // Every MATCHED pair `rank` is a party to becomes CLAIMED by it, in match order per list walk
  void claim(int rank, std::vector<std::shared_ptr<P2PPair>>* out) {
    out->clear();
    std::lock_guard<std::mutex> g(mu_);
    for (auto it = matched_.begin(); it != matched_.end();) {
      P2PPair& p = **it;
      if (p.state == kPairMatched && (p.s->rank == rank || p.r->rank == rank)) {
        p.state = kPairClaimed;
        p.mover = rank;
        out->push_back(*it);
        it = matched_.erase(it);
      } else {
        ++it;
      }
    }
  }

  // The batch was enqueued (err == kP2POk: `done` is its completion event) or could not be
  void launched(const std::vector<std::shared_ptr<P2PPair>>& batch, const std::shared_ptr<void>& done, int err = kP2POk,
                const std::string& msg = std::string()) {
    {
      std::lock_guard<std::mutex> g(mu_);
      for (const auto& p : batch) {
        p->done = done;
        p->err = err;
        p->msg = msg;
        p->state = err == kP2POk ? kPairLaunched : kPairFailed;
      }
    }
    cv_.notify_all();
  }

  enum Wake { kWakeSettled, kWakeMatched, kWakeTimeout, kWakeFailed };
  // Sleeps until q is LAUNCHED or FAILED (settled), or MATCHED and unclaimed (the caller claims it), until
  // `deadline`, or until *failed (the world's flag, observed at least every 50 ms) is set.
  Wake wait(const std::shared_ptr<P2PReq>& q, Clock::time_point deadline, const std::atomic<int>* failed) {
    std::unique_lock<std::mutex> lk(mu_);
    for (;;) {
      if (q->null_peer || q->orphan) return kWakeSettled;
      if (q->pair) {
        const int st = q->pair->state;
        if (st == kPairLaunched || st == kPairFailed) return kWakeSettled;
        if (st == kPairMatched) return kWakeMatched;
      }
      if (failed && failed->load(std::memory_order_acquire)) return kWakeFailed;
      const auto now = Clock::now();
      if (now >= deadline) return kWakeTimeout;
      const auto slice = std::min<Clock::duration>(deadline - now, std::chrono::milliseconds(50));
      // a slice on the system clock (pthread_cond_timedwait, which ThreadSanitizer intercepts); the deadline itself
      // is on the steady clock
      cv_.wait_until(lk, std::chrono::system_clock::now() + slice);
    }
  }

  // The state of q for a call that does not sleep
  bool settled(const std::shared_ptr<P2PReq>& q) {
    std::lock_guard<std::mutex> g(mu_);
    if (q->null_peer || q->orphan) return true;
    return q->pair && (q->pair->state == kPairLaunched || q->pair->state == kPairFailed);
  }

  // q leaves the lists unmatched (its wait gave up, or mpjx_request_free); false if it was matched already
  bool withdraw(const std::shared_ptr<P2PReq>& q) {
    std::lock_guard<std::mutex> g(mu_);
    if (q->pair || q->null_peer) return false;
    q->orphan = true;
    for (auto* lists : {&recvs_, &sends_})
      for (auto& l : *lists)
        for (auto it = l.begin(); it != l.end(); ++it)
          if (it->get() == q.get()) {
            l.erase(it);
            return true;
          }
    return true;
  }

  // The communicator of `rank` is destroyed: its unmatched requests leave the lists and its unmoved pairs
  // fail on both sides (nothing is moved into or out of memory the caller is about to free)
  void retire_rank(int rank) {
    {
      std::lock_guard<std::mutex> g(mu_);
      for (auto* lists : {&recvs_, &sends_})
        for (auto& l : *lists)
          for (auto it = l.begin(); it != l.end();)
            if ((*it)->rank == rank) {
              (*it)->orphan = true;
              it = l.erase(it);
            } else {
              ++it;
            }
      for (auto it = matched_.begin(); it != matched_.end();) {
        P2PPair& p = **it;
        if (p.s->rank == rank || p.r->rank == rank) {
          p.state = kPairFailed;
          p.err = kP2PErrInternal;
          p.msg = "the communicator of rank " + std::to_string(rank) + " was destroyed with " + p.s->envelope() +
                  " matched to " + p.r->envelope() + " still pending";
          it = matched_.erase(it);
        } else {
          ++it;
        }
      }
    }
    cv_.notify_all();
  }

  // The caller is done with q (its status was read, or it is freed): q lets go of its pair. A pair and its two
  // requests refer to each other, so the pair lives until both requests have been released.
  void release(const std::shared_ptr<P2PReq>& q) {
    std::shared_ptr<P2PPair> drop;
    std::lock_guard<std::mutex> g(mu_);
    drop.swap(q->pair);
    if (drop && !q->send && drop->s->eager) {  // nobody else releases an eager send
      drop->s->consumed = true;
      drop->s->pair.reset();
    }
  }

  // Probe: the first unmatched send addressed to `rank`, in post order, that a receive (source, tag) posted now
  // would match; wildcards honoured, eager sends included. Nothing is consumed. *st gets its source, tag, packed
  // bytes (a PACKED send: image bytes) and elements (bytes / bsz, or kUndefined for a PACKED send, whose header
  // the host cannot know).
  bool peek(int rank, int source, int tag, P2PStatus* st) {
    std::lock_guard<std::mutex> g(mu_);
    return peek_locked(rank, source, tag, st);
  }
  // Sleeps until peek succeeds (kWakeMatched), until `deadline`, or until *failed is set, as wait does
  Wake probe(int rank, int source, int tag, Clock::time_point deadline, const std::atomic<int>* failed, P2PStatus* st) {
    std::unique_lock<std::mutex> lk(mu_);
    struct Count {
      int& n;
      explicit Count(int& x) : n(x) { ++n; }
      ~Count() { --n; }
    } probing(probers_);
    for (;;) {
      if (peek_locked(rank, source, tag, st)) return kWakeMatched;
      if (failed && failed->load(std::memory_order_acquire)) return kWakeFailed;
      const auto now = Clock::now();
      if (now >= deadline) return kWakeTimeout;
      const auto slice = std::min<Clock::duration>(deadline - now, std::chrono::milliseconds(50));
      cv_.wait_until(lk, std::chrono::system_clock::now() + slice);
    }
  }

  // The result slot of an unpack pair was read after its batch's completion event passed: n base elements, or a
  // nonzero MPJX_MPJBUF_* code, which completes the pair with MPJX_ERR_ARG on every party still waiting. The
  // first call counts; both parties read the same slot.
  void resolve(P2PPair& p, int code, int64_t n) {
    std::lock_guard<std::mutex> g(mu_);
    if (p.resolved) return;
    p.resolved = true;
    p.wire_n = code == 0 ? n : 0;
    if (code != 0 && p.err == kP2POk) {
      static const char* const names[] = {"", "MPJX_MPJBUF_BAD_TYPE", "MPJX_MPJBUF_BAD_COUNT", "MPJX_MPJBUF_OVERRUN"};
      p.err = kP2PErrArg;
      p.msg = std::string("the image's first section cannot be received (") + (code >= 1 && code <= 3 ? names[code] : "?") +
              ", code " + std::to_string(code) + ", header count " + std::to_string(n) + "): " + p.s->envelope() +
              " matched " + p.r->envelope();
    }
  }

  void notify() { cv_.notify_all(); }
  std::mutex& mutex() { return mu_; }  // the eager slab is handed out under the mailbox lock

  // counts of unmatched requests (tests)
  size_t pending() {
    std::lock_guard<std::mutex> g(mu_);
    size_t n = 0;
    for (auto& l : recvs_) n += l.size();
    for (auto& l : sends_) n += l.size();
    return n;
  }

 private:
  // post's body (mu_ held)
  std::shared_ptr<P2PPair> post_locked(const std::shared_ptr<P2PReq>& q) {
    std::shared_ptr<P2PPair> made;
    if (q->peer == kProcNull) {
      q->null_peer = true;
      return nullptr;
    }
    const int dst = q->send ? q->peer : q->rank;
    auto& mine = q->send ? sends_[(size_t)dst] : recvs_[(size_t)dst];
    auto& other = q->send ? recvs_[(size_t)dst] : sends_[(size_t)dst];
    for (auto it = other.begin(); it != other.end(); ++it) {
      const P2PReq& s = q->send ? *q : **it;
      const P2PReq& r = q->send ? **it : *q;
      if ((r.peer == kAnySource || r.peer == s.rank) && (r.tag == kAnyTag || r.tag == s.tag)) {
        made = std::make_shared<P2PPair>();
        made->s = q->send ? q : *it;
        made->r = q->send ? *it : q;
        other.erase(it);
        break;
      }
    }
    if (!made) {
      mine.push_back(q);
      return nullptr;
    }
    made->s->pair = made;
    made->r->pair = made;
    if (check(*made)) matched_.push_back(made);
    return made;
  }

  // The checks at match time (mu_ held); false for a pair that is FAILED
  bool check(P2PPair& p) {
    const P2PReq &s = *p.s, &r = *p.r;
    auto bad = [&](const std::string& why) {
      p.state = kPairFailed;
      p.err = kP2PErrArg;
      p.msg = why + ": " + s.envelope() + " matched " + r.envelope();
    };
    // The base-type test passes when either side is PACKED (Comm.java:394-407, :1460-1474)
    const bool sp = s.base == kP2PPacked, rp = r.base == kP2PPacked;
    if (sp != rp) {
      const P2PReq& typed = sp ? r : s;
      if (typed.bsz > 1 && typed.lay.base % (uint64_t)typed.bsz) {
        bad("the typed buffer of a message with MPI.PACKED on the other side is not aligned to its " +
            std::to_string(typed.bsz) + "-byte base element");
        return false;
      }
      if (rp) {  // pack on the fly: one section at position 0 of the receiver's image
        const int64_t words = s.bytes / (s.bsz > 0 ? s.bsz : 1);
        if (words > 0x7fffffff) {
          bad(std::to_string(words) + " base elements exceed the section header's int32 count (2^31 - 1)");
          return false;
        }
        if (8 + s.bytes > r.bytes) {
          bad("the section of 8 header and " + std::to_string(s.bytes) + " payload bytes is longer than the image of " +
              std::to_string(r.bytes));
          return false;
        }
        p.wire = kPairPack;
      } else {  // unpack on the fly: the kernel reads the header; the host knows only the image's length
        if (s.bytes < 8) {
          bad("an image of " + std::to_string(s.bytes) + " bytes holds no section header");
          return false;
        }
        p.wire = kPairUnpack;
      }
    } else if (s.bytes > 0 && s.base != r.base) {
      bad("base type " + std::to_string(s.base) + " sent, base type " + std::to_string(r.base) + " received");
      return false;
    }
    if (p.wire == kPairPlain && s.bytes > r.bytes) {
      bad("the message of " + std::to_string(s.bytes) + " packed bytes is longer than the receive layout of " +
          std::to_string(r.bytes));
      return false;
    }
    if (s.rank == r.rank && s.bytes > 0) {
      int a = 0, b = 0;
      const OverlapResult o = strided_overlap({s.lay}, {r.lay}, &a, &b);
      if (o == kSendRecvOverlap || o == kRecvOverlap) {
        bad("a self-message whose send and receive layouts share a byte");
        return false;
      }
    }
    return true;
  }

  // peek's body (mu_ held)
  bool peek_locked(int rank, int source, int tag, P2PStatus* st) const {
    for (const auto& sp : sends_[(size_t)rank]) {
      const P2PReq& s = *sp;
      if ((source == kAnySource || source == s.rank) && (tag == kAnyTag || tag == s.tag)) {
        *st = P2PStatus{};
        st->source = s.rank;
        st->tag = s.tag;
        st->bytes = s.bytes;
        st->elements = s.base == kP2PPacked ? kUndefined : s.bytes / (s.bsz > 0 ? s.bsz : 1);
        return true;
      }
    }
    return false;
  }

  int probers_ = 0;  // calls asleep in probe (mu_ held): post then wakes them for an unmatched send as well
  std::mutex mu_;
  std::condition_variable cv_;
  std::vector<std::deque<std::shared_ptr<P2PReq>>> recvs_, sends_;
  std::deque<std::shared_ptr<P2PPair>> matched_;
  int P_;
};

// ---- persistent requests (src/mpi/Prequest.java) ------------------------------------------------------------------

// The checked plan of a send or a receive, made once by Send_init / Recv_init, and its current activation. Start
// makes a fresh P2PReq from the plan, which the mailbox sees as an Isend or Irecv posted now; completion (or a
// failed wait, or Free) makes the request inactive again. The serial is unique in the process and never reused:
// it keys the device segment pool (mpjx_msgs_pool_plan.hpp). Not thread-safe: a request belongs to its rank's
// thread, as every mpjx_request does.
struct Persist {
  P2PReq plan;                  // never posted itself: no pair, no ready event
  std::shared_ptr<P2PReq> act;  // the pending activation; none while inactive

  explicit Persist(const P2PReq& p) : plan(p) {
    static std::atomic<uint64_t> next{1};
    plan.serial = next.fetch_add(1, std::memory_order_relaxed);
    plan.freed = std::make_shared<std::atomic<bool>>(false);
    plan.pair.reset();
    plan.ready.reset();
  }
  ~Persist() { plan.freed->store(true, std::memory_order_release); }
  uint64_t serial() const { return plan.serial; }
  bool active() const { return (bool)act; }
  // The activation to post, or none if the request is active already
  std::shared_ptr<P2PReq> start() {
    if (act) return nullptr;
    act = std::make_shared<P2PReq>(plan);
    return act;
  }
  // The activation leaves the mailbox (unmatched: withdrawn; matched: its pair is let go) and the request is
  // inactive. What a completed wait, a failed one and Free do.
  void finish(Mailbox* mb) {
    if (!act) return;
    if (mb) {
      mb->withdraw(act);
      mb->release(act);
    }
    act.reset();
  }
};

// ---- the eager slab -------------------------------------------------------------------------------------------

// First-fit allocator over `cap` bytes in chunks aligned to 256 B. A chunk carries the request of the message
// packed into it and is released once `done(request)` says its message has been moved, checked at the next
// allocation. Not thread-safe: its rank calls it under the mailbox lock.
class EagerSlab {
 public:
  static constexpr int64_t kAlign = 256;
  explicit EagerSlab(int64_t cap = 0) : cap_(cap) {}
  int64_t capacity() const { return cap_; }
  size_t live() const { return chunks_.size(); }
  // The offset of a chunk of `bytes` (> 0) for `owner`, or -1 when no gap is large enough
  template <class Done>
  int64_t alloc(int64_t bytes, const std::shared_ptr<P2PReq>& owner, Done done) {
    for (auto it = chunks_.begin(); it != chunks_.end();) it = done(it->owner) ? chunks_.erase(it) : it + 1;
    const int64_t need = (bytes + kAlign - 1) / kAlign * kAlign;
    int64_t at = 0;
    auto it = chunks_.begin();
    for (; it != chunks_.end(); ++it) {  // sorted by offset
      if (it->off - at >= need) break;
      at = it->off + it->len;
    }
    if (it == chunks_.end() && cap_ - at < need) return -1;
    chunks_.insert(it, Chunk{at, need, owner});
    return at;
  }
  // Drops every chunk, handing its owner to f first
  template <class F>
  void clear(F f) {
    for (Chunk& c : chunks_) f(c.owner);
    chunks_.clear();
  }

 private:
  struct Chunk {
    int64_t off, len;
    std::shared_ptr<P2PReq> owner;
  };
  std::vector<Chunk> chunks_;
  int64_t cap_;
};

}  // namespace mpjx
