// CPU test of Probe / Iprobe's host side and of the matching of MPI.PACKED messages
// (mpjexpress_amd/csrc/mpjx_p2p_plan.hpp: Mailbox::peek, probe, resolve and check): plain C++17, no HIP. Built by
// the Makefile with g++, and by tests/test_wire_abi.py under -fsanitize=address,undefined and -fsanitize=thread.
//   - peek: post order, wildcards, the destination, eager sends; it does not consume; of two sends the first is
//     seen (non-overtaking); the status of a typed and of a PACKED send
//   - probe: sleeps until a send is posted, ends at its deadline and on the world's failed flag
//   - 8 threads: probes and peeks race with post, every message is still received exactly once
//   - check: typed/PACKED pairs pass and are marked for k_wire; an undersized image, a PACKED send of fewer than 8
//     bytes to a typed receive and a misaligned typed buffer fail; the statuses of the three receive kinds
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>

#include "../../mpjexpress_amd/csrc/mpjx_p2p_plan.hpp"

using namespace mpjx;

static std::atomic<int> g_fail{0};
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      g_fail++;                                                  \
    }                                                            \
  } while (0)

using Req = std::shared_ptr<P2PReq>;

static SideBytes run(uint64_t base, int64_t bytes) {
  SideBytes x;
  x.base = base;
  x.bb = x.sb = x.eb = bytes;
  x.nb = x.items = bytes > 0 ? 1 : 0;
  return x;
}

// base 5 (INT, 4-byte words) unless PACKED (1-byte words)
static Req mk(bool send, int rank, int peer, int tag, int64_t bytes = 8, int base = 5, uint64_t addr = 0) {
  auto q = std::make_shared<P2PReq>();
  q->send = send;
  q->rank = rank;
  q->peer = peer;
  q->tag = tag;
  q->base = base;
  q->bsz = base == kP2PPacked ? 1 : base == 8 ? 8 : 4;
  q->bytes = bytes;
  q->lay = run(addr ? addr : (uint64_t)(0x10000 + 0x1000 * rank + (send ? 0 : 0x800)), bytes);
  return q;
}

static Mailbox::Clock::time_point in_ms(int ms) { return Mailbox::Clock::now() + std::chrono::milliseconds(ms); }

static void test_peek() {
  Mailbox mb(3);
  P2PStatus st;
  CHECK(!mb.peek(1, kAnySource, kAnyTag, &st));
  Req a = mk(true, 0, 1, 7, 40), b = mk(true, 0, 1, 7, 80), c = mk(true, 2, 1, 9, 24, kP2PPacked), d = mk(true, 0, 2, 7, 8);
  c->eager = true;  // an eager send is seen like any other
  for (const Req& q : {a, b, c, d}) CHECK(!mb.post(q));
  // of two sends of one envelope the first is seen, again and again: nothing is consumed
  for (int i = 0; i < 3; i++) {
    CHECK(mb.peek(1, 0, 7, &st) && st.source == 0 && st.tag == 7 && st.bytes == 40 && st.elements == 10 && st.error == 0);
    CHECK(mb.peek(1, kAnySource, kAnyTag, &st) && st.bytes == 40);
    CHECK(mb.peek(1, kAnySource, 7, &st) && st.bytes == 40 && mb.peek(1, 0, kAnyTag, &st) && st.bytes == 40);
  }
  CHECK(mb.pending() == 4);
  // a PACKED send: the image's bytes, elements unknown to the host
  CHECK(mb.peek(1, 2, kAnyTag, &st) && st.source == 2 && st.tag == 9 && st.bytes == 24 && st.elements == kUndefined);
  CHECK(mb.peek(1, kAnySource, 9, &st) && st.source == 2);
  CHECK(!mb.peek(1, 2, 7, &st) && !mb.peek(1, 0, 9, &st) && !mb.peek(1, 1, kAnyTag, &st));
  CHECK(mb.peek(2, kAnySource, kAnyTag, &st) && st.source == 0 && st.bytes == 8 && !mb.peek(0, kAnySource, kAnyTag, &st));
  // a receive takes the message the probe saw; the next probe sees the second
  Req r = mk(false, 1, kAnySource, kAnyTag, 400);
  auto p = mb.post(r);
  CHECK(p && p->s == a && p->state == kPairMatched);
  CHECK(mb.peek(1, 0, 7, &st) && st.bytes == 80);
  // a posted receive hides nothing and is never seen itself
  Req r2 = mk(false, 0, 1, 3);
  CHECK(!mb.post(r2) && !mb.peek(0, kAnySource, kAnyTag, &st) && !mb.peek(1, 1, 3, &st));
  mb.withdraw(r2);
  for (const Req& q : {b, c, d}) mb.withdraw(q);
  mb.release(r);
  mb.release(a);
}

static void test_probe_waits() {
  Mailbox mb(2);
  P2PStatus st;
  std::atomic<int> failed{0};
  // nothing comes: the deadline ends it
  const auto t0 = Mailbox::Clock::now();
  CHECK(mb.probe(1, 0, 5, in_ms(120), &failed, &st) == Mailbox::kWakeTimeout);
  CHECK(Mailbox::Clock::now() - t0 >= std::chrono::milliseconds(100));
  // a send posted while it sleeps wakes it
  Req s = mk(true, 0, 1, 5, 16);
  std::thread poster([&] {
    std::this_thread::sleep_for(std::chrono::milliseconds(30));
    mb.post(s);
  });
  CHECK(mb.probe(1, kAnySource, kAnyTag, in_ms(5000), &failed, &st) == Mailbox::kWakeMatched);
  CHECK(st.source == 0 && st.tag == 5 && st.bytes == 16 && st.elements == 4);
  poster.join();
  CHECK(mb.pending() == 1);
  // the world's flag ends a probe that nothing matches
  std::thread failer([&] {
    std::this_thread::sleep_for(std::chrono::milliseconds(30));
    failed.store(1, std::memory_order_release);
    mb.notify();
  });
  CHECK(mb.probe(1, 0, 6, in_ms(5000), &failed, &st) == Mailbox::kWakeFailed);
  failer.join();
  mb.withdraw(s);
}

// 4 senders and 4 receivers on 8 threads: every receiver probes (blocking or polling) before each receive, and
// other probes run beside it; each message is received exactly once and in order per sender
static void test_races() {
  constexpr int kPairs = 4, kMsgs = 1500;
  Mailbox mb(2 * kPairs);
  std::atomic<int> failed{0};
  std::atomic<long> received{0};
  std::vector<std::thread> th;
  for (int i = 0; i < kPairs; i++) {
    th.emplace_back([&, i] {  // sender rank i -> receiver rank kPairs + i
      for (int m = 0; m < kMsgs; m++) {
        Req s = mk(true, i, kPairs + i, m % 50, 8 + 4 * (m % 7));
        mb.post(s);
        P2PStatus st;
        (void)mb.peek(kPairs + (i + 1) % kPairs, kAnySource, kAnyTag, &st);  // peeks at another rank's list
      }
    });
    th.emplace_back([&, i] {
      const int me = kPairs + i;
      for (int m = 0; m < kMsgs; m++) {
        P2PStatus st;
        if (m % 2) {
          while (!mb.peek(me, kAnySource, kAnyTag, &st)) std::this_thread::yield();
        } else {
          CHECK(mb.probe(me, i, kAnyTag, in_ms(20000), &failed, &st) == Mailbox::kWakeMatched);
        }
        CHECK(st.source == i && st.tag == m % 50 && st.bytes == 8 + 4 * (m % 7));  // the next one in order
        Req r = mk(false, me, st.source, st.tag, 64);
        auto p = mb.post(r);
        CHECK(p && p->state == kPairMatched && p->s->bytes == st.bytes);  // the receive takes what the probe saw
        std::vector<std::shared_ptr<P2PPair>> batch;
        mb.claim(me, &batch);
        mb.launched(batch, nullptr);
        received += (long)batch.size();
        mb.release(p->s);
        mb.release(r);
      }
    });
  }
  for (auto& t : th) t.join();
  CHECK(received.load() == (long)kPairs * kMsgs && mb.pending() == 0);
}

// A pair and its two requests refer to each other until both are released: test_check lets them go at its end
static std::vector<Req> g_made;
static std::shared_ptr<P2PPair> pair_of(Mailbox& mb, const Req& s, const Req& r) {
  g_made.push_back(s);
  g_made.push_back(r);
  CHECK(!mb.post(r));
  return mb.post(s);
}

static void test_check() {
  Mailbox mb(2);
  const int P = kP2PPacked;
  // typed -> PACKED: the room holds the header and the payload
  {
    Req s = mk(true, 0, 1, 1, 40), r = mk(false, 1, 0, 1, 48, P);
    auto p = pair_of(mb, s, r);
    CHECK(p && p->state == kPairMatched && p->wire == kPairPack && p->err == kP2POk);
    const P2PStatus rs = p2p_status(*r), ss = p2p_status(*s);
    CHECK(rs.bytes == 48 && rs.elements == 48 && rs.source == 0 && rs.tag == 1);
    CHECK(ss.bytes == 40 && ss.elements == 10);  // the sender's own packed bytes
  }
  {  // one byte short
    Req s = mk(true, 0, 1, 2, 40), r = mk(false, 1, 0, 2, 47, P);
    auto p = pair_of(mb, s, r);
    CHECK(p && p->state == kPairFailed && p->err == kP2PErrArg && p->msg.find("longer than the image of 47") != std::string::npos);
    CHECK(p->msg.find("send(rank 0 -> 1") != std::string::npos && p->msg.find("recv(rank 1 <- 0") != std::string::npos);
  }
  {  // 0 items still need the header's room
    Req s = mk(true, 0, 1, 3, 0), r8 = mk(false, 1, 0, 3, 8, P);
    auto p = pair_of(mb, s, r8);
    CHECK(p && p->state == kPairMatched && p->wire == kPairPack && p2p_status(*r8).bytes == 8);
    Req s2 = mk(true, 0, 1, 4, 0), r0 = mk(false, 1, 0, 4, 0, P);
    auto p2 = pair_of(mb, s2, r0);
    CHECK(p2 && p2->state == kPairFailed);
  }
  // PACKED -> typed: the host knows only the image's length
  {
    Req s = mk(true, 0, 1, 5, 8 + 400, P), r = mk(false, 1, 0, 5, 40);  // longer than the room: the kernel decides
    auto p = pair_of(mb, s, r);
    CHECK(p && p->state == kPairMatched && p->wire == kPairUnpack);
    p->state = kPairLaunched;
    mb.resolve(*p, 0, 7);
    mb.resolve(*p, 3, 99);  // the first reading counts
    const P2PStatus rs = p2p_status(*r);
    CHECK(rs.error == kP2POk && rs.elements == 7 && rs.bytes == 28 && p2p_status(*s).bytes == 408);
  }
  {
    Req s = mk(true, 0, 1, 6, 7, P), r = mk(false, 1, 0, 6, 40);
    auto p = pair_of(mb, s, r);
    CHECK(p && p->state == kPairFailed && p->err == kP2PErrArg && p->msg.find("no section header") != std::string::npos);
    Req s4 = mk(true, 0, 1, 6, 4, P), r4 = mk(false, 1, 0, 6, 40);
    CHECK(pair_of(mb, s4, r4)->state == kPairFailed);
  }
  {  // a device-found error completes the pair with MPJX_ERR_ARG and names the code and both envelopes
    Req s = mk(true, 0, 1, 7, 16, P), r = mk(false, 1, 0, 7, 40);
    auto p = pair_of(mb, s, r);
    p->state = kPairLaunched;
    mb.resolve(*p, 1, 2);
    const P2PStatus rs = p2p_status(*r);
    CHECK(rs.error == kP2PErrArg && rs.elements == 0 && rs.bytes == 0);
    CHECK(p->msg.find("MPJX_MPJBUF_BAD_TYPE") != std::string::npos && p->msg.find("send(rank 0") != std::string::npos &&
          p->msg.find("recv(rank 1") != std::string::npos);
  }
  {  // the typed side must be element-aligned
    Req s = mk(true, 0, 1, 8, 16, P), r = mk(false, 1, 0, 8, 40, 5, 0x20002);
    CHECK(pair_of(mb, s, r)->state == kPairFailed);
  }
  // PACKED -> PACKED: a byte message; longer than the room fails, 0 bytes is an empty message
  {
    Req s = mk(true, 0, 1, 9, 24, P), r = mk(false, 1, 0, 9, 32, P);
    auto p = pair_of(mb, s, r);
    CHECK(p && p->state == kPairMatched && p->wire == kPairPlain);
    const P2PStatus rs = p2p_status(*r);
    CHECK(rs.bytes == 24 && rs.elements == 24);
    Req s2 = mk(true, 0, 1, 9, 33, P), r2 = mk(false, 1, 0, 9, 32, P);
    CHECK(pair_of(mb, s2, r2)->state == kPairFailed);
    Req s3 = mk(true, 0, 1, 9, 0, P), r3 = mk(false, 1, 0, 9, 0, P);
    auto p3 = pair_of(mb, s3, r3);
    CHECK(p3 && p3->state == kPairMatched && p2p_status(*r3).bytes == 0);
  }
  {  // typed pairs are as they were: a base-type mismatch fails, equal types pass unmarked
    Req s = mk(true, 0, 1, 10, 16, 5), r = mk(false, 1, 0, 10, 16, 8);
    CHECK(pair_of(mb, s, r)->state == kPairFailed);
    Req s2 = mk(true, 0, 1, 10, 16, 5), r2 = mk(false, 1, 0, 10, 16, 5);
    auto p = pair_of(mb, s2, r2);
    CHECK(p->state == kPairMatched && p->wire == kPairPlain);
  }
  // p2p_get_count with MPI.PACKED's size of 1
  int64_t cn = 0, el = 0;
  p2p_get_count(48, 1, &cn, &el);
  CHECK(cn == 48 && el == 48);
  for (const Req& q : g_made) mb.release(q);
  g_made.clear();
}

int main() {
  test_peek();
  test_probe_waits();
  test_races();
  test_check();
  if (g_fail) {
    printf("p2p_probe_test: %d failure(s)\n", g_fail.load());
    return 1;
  }
  printf("p2p_probe_test: ok\n");
  return 0;
}
