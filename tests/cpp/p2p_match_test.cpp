// CPU test of the point-to-point matching engine and the eager slab (mpjexpress_amd/csrc/mpjx_p2p_plan.hpp):
// plain C++17, no HIP. Built by the Makefile with g++, and by tests/test_p2p_abi.py under
// -fsanitize=address,undefined and -fsanitize=thread.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <random>
#include <thread>

#include "../../mpjexpress_amd/csrc/mpjx_p2p_plan.hpp"

using namespace mpjx;

static int g_fail = 0;
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

static Req mk(bool send, int rank, int peer, int tag, int64_t bytes = 8, int base = 5, uint64_t addr = 0) {
  auto q = std::make_shared<P2PReq>();
  q->send = send;
  q->rank = rank;
  q->peer = peer;
  q->tag = tag;
  q->base = base;
  q->bsz = 4;
  q->bytes = bytes;
  q->lay = run(addr ? addr : (uint64_t)(0x10000 + 0x1000 * rank + (send ? 0 : 0x800)), bytes);
  return q;
}

static void release_all(Mailbox& mb, std::initializer_list<Req> l) {
  for (const Req& q : l) mb.release(q);
}

static void test_post_order() {
  Mailbox mb(2);
  Req r1 = mk(false, 1, 0, 7), r2 = mk(false, 1, 0, 7), s1 = mk(true, 0, 1, 7), s2 = mk(true, 0, 1, 7);
  CHECK(!mb.post(r1) && !mb.post(r2));
  auto p1 = mb.post(s1);
  auto p2 = mb.post(s2);
  CHECK(p1 && p1->r == r1 && p1->s == s1 && p1->state == kPairMatched);
  CHECK(p2 && p2->r == r2 && p2->s == s2);
  CHECK(mb.pending() == 0);
  // sends first, then receives: the first unmatched send wins
  Req s3 = mk(true, 0, 1, 9), s4 = mk(true, 0, 1, 9), r3 = mk(false, 1, 0, 9);
  mb.post(s3);
  mb.post(s4);
  auto p3 = mb.post(r3);
  CHECK(p3 && p3->s == s3 && mb.pending() == 1);
  // a send to another destination does not match
  Req s5 = mk(true, 1, 0, 9), r5 = mk(false, 1, 0, 9);
  CHECK(!mb.post(s5));
  auto p5 = mb.post(r5);
  CHECK(p5 && p5->s == s4);
  const P2PStatus st = p2p_status(*r5);
  CHECK(st.source == 0 && st.tag == 9 && st.bytes == 8 && st.elements == 2 && st.error == 0);
  mb.withdraw(s5);
  release_all(mb, {r1, r2, s1, s2, s3, s4, r3, r5, s5});
}

static void test_wildcards() {
  for (int ws = 0; ws < 2; ws++)
    for (int wt = 0; wt < 2; wt++) {
      Mailbox mb(3);
      Req r = mk(false, 2, ws ? kAnySource : 1, wt ? kAnyTag : 5);
      mb.post(r);
      Req wrong_src = mk(true, 0, 2, 5), wrong_tag = mk(true, 1, 2, 6), right = mk(true, 1, 2, 5);
      std::shared_ptr<P2PPair> p;
      if (!ws) CHECK(!mb.post(wrong_src));
      if (!wt) CHECK(!mb.post(wrong_tag));
      Req first = ws ? wrong_src : (wt ? wrong_tag : right);
      if (ws) {
        p = mb.post(wrong_src);
        CHECK(p && p->s == wrong_src);
      } else if (wt) {
        p = mb.post(wrong_tag);
        CHECK(p && p->s == wrong_tag);
      } else {
        p = mb.post(right);
        CHECK(p && p->s == right);
      }
      const P2PStatus st = p2p_status(*r);
      CHECK(st.source == first->rank && st.tag == first->tag);
      for (const Req& q : {wrong_src, wrong_tag, right, r}) {
        mb.withdraw(q);
        mb.release(q);
      }
    }
}

static void test_proc_null() {
  Mailbox mb(2);
  Req s = mk(true, 0, kProcNull, 3), r = mk(false, 0, kProcNull, kAnyTag);
  CHECK(!mb.post(s) && !mb.post(r));
  CHECK(s->null_peer && r->null_peer && mb.pending() == 0 && mb.settled(s) && mb.settled(r));
  const P2PStatus st = p2p_status(*r);
  CHECK(st.source == kProcNull && st.tag == kAnyTag && st.elements == 0 && st.bytes == 0 && st.error == 0);
  std::atomic<int> failed{0};
  CHECK(mb.wait(r, Mailbox::Clock::now(), &failed) == Mailbox::kWakeSettled);
}

static void test_non_overtaking() {
  // tags interleaved 1 2 1 2 ...: receives by tag take the sends of that tag in send order; ANY_TAG takes them
  // in send order
  Mailbox mb(2);
  std::vector<Req> sends;
  for (int i = 0; i < 8; i++) {
    sends.push_back(mk(true, 0, 1, 1 + i % 2, 8 + 4 * i));
    mb.post(sends.back());
  }
  std::vector<Req> all(sends);
  for (int k = 0; k < 2; k++) {
    Req r = mk(false, 1, 0, 2, 64);
    auto p = mb.post(r);
    CHECK(p && p->s == sends[(size_t)(1 + 2 * k)]);
    all.push_back(r);
  }
  const int expect[6] = {0, 2, 4, 5, 6, 7};
  for (int k = 0; k < 6; k++) {
    Req r = mk(false, 1, kAnySource, kAnyTag, 64);
    auto p = mb.post(r);
    CHECK(p && p->s == sends[(size_t)expect[k]]);
    all.push_back(r);
  }
  CHECK(mb.pending() == 0);
  for (const Req& q : all) mb.release(q);
}

static void test_checks() {
  Mailbox mb(2);
  // shorter accepted
  Req r = mk(false, 1, 0, 1, 64), s = mk(true, 0, 1, 1, 12);
  mb.post(r);
  auto p = mb.post(s);
  CHECK(p && p->state == kPairMatched && p->err == 0);
  CHECK(p2p_status(*r).elements == 3 && p2p_status(*r).bytes == 12);
  // over-long rejected on both, the message names both envelopes, and nothing is left to claim
  Req r2 = mk(false, 1, 0, 2, 8), s2 = mk(true, 0, 1, 2, 12);
  mb.post(s2);
  auto p2 = mb.post(r2);
  CHECK(p2 && p2->state == kPairFailed && p2->err == kP2PErrArg);
  CHECK(p2->msg.find("send(rank 0 -> 1, tag 2, 12 B)") != std::string::npos);
  CHECK(p2->msg.find("recv(rank 1 <- 0, tag 2, 8 B)") != std::string::npos);
  CHECK(p2p_status(*r2).error == kP2PErrArg && p2p_status(*s2).error == kP2PErrArg && mb.settled(r2) && mb.settled(s2));
  // base-type mismatch
  Req r3 = mk(false, 1, 0, 3, 8, 5), s3 = mk(true, 0, 1, 3, 8, 8);
  mb.post(r3);
  auto p3 = mb.post(s3);
  CHECK(p3 && p3->state == kPairFailed && p3->msg.find("base type 8 sent, base type 5 received") != std::string::npos);
  // an empty message matches whatever the base types
  Req r4 = mk(false, 1, 0, 4, 8, 5), s4 = mk(true, 0, 1, 4, 0, 8);
  mb.post(r4);
  CHECK(mb.post(s4)->state == kPairMatched);
  // a self-message whose layouts share a byte
  Req r5 = mk(false, 0, 0, 5, 16, 5, 0x5000), s5 = mk(true, 0, 0, 5, 16, 5, 0x5008);
  mb.post(r5);
  CHECK(mb.post(s5)->state == kPairFailed);
  Req r6 = mk(false, 0, 0, 6, 16, 5, 0x6000), s6 = mk(true, 0, 0, 6, 16, 5, 0x6010);
  mb.post(r6);
  CHECK(mb.post(s6)->state == kPairMatched);
  // only the good pairs are claimed, by either party, exactly once; the world stays usable
  std::vector<std::shared_ptr<P2PPair>> got;
  mb.claim(1, &got);
  CHECK(got.size() == 2 && got[0] == p && got[0]->state == kPairClaimed && got[0]->mover == 1);
  mb.claim(0, &got);
  CHECK(got.size() == 1 && got[0]->s == s6);
  mb.launched(got, nullptr);
  CHECK(mb.settled(r6) && mb.settled(s6) && !mb.settled(r));
  mb.claim(0, &got);
  CHECK(got.empty());
  release_all(mb, {r, s, r2, s2, r3, s3, r4, s4, r5, s5, r6, s6});
}

static void test_wait_and_retire() {
  Mailbox mb(2);
  std::atomic<int> failed{0};
  Req r = mk(false, 1, 0, 1);
  mb.post(r);
  const auto t0 = Mailbox::Clock::now();
  CHECK(mb.wait(r, t0 + std::chrono::milliseconds(30), &failed) == Mailbox::kWakeTimeout);
  CHECK(Mailbox::Clock::now() - t0 >= std::chrono::milliseconds(30));
  failed.store(1);
  CHECK(mb.wait(r, t0 + std::chrono::seconds(30), &failed) == Mailbox::kWakeFailed);
  failed.store(0);
  std::thread th([&] { mb.post(mk(true, 0, 1, 1)); });
  CHECK(mb.wait(r, Mailbox::Clock::now() + std::chrono::seconds(30), &failed) == Mailbox::kWakeMatched);
  th.join();
  Req sender = r->pair->s;
  mb.retire_rank(0);  // the sender's communicator goes away with the pair unmoved
  CHECK(mb.settled(r) && p2p_status(*r).error == kP2PErrInternal);
  Req r2 = mk(false, 1, 0, 2);
  mb.post(r2);
  mb.retire_rank(1);
  CHECK(r2->orphan && mb.pending() == 0);
  release_all(mb, {r, sender, r2});
}

static void test_slab() {
  EagerSlab slab(4096);
  std::vector<Req> q;
  for (int i = 0; i < 8; i++) q.push_back(mk(true, 0, 1, i));
  auto done = [](const Req& x) { return x->consumed; };
  CHECK(slab.alloc(1, q[0], done) == 0);      // rounded up to 256
  CHECK(slab.alloc(300, q[1], done) == 256);  // 512
  CHECK(slab.alloc(256, q[2], done) == 768);
  CHECK(slab.alloc(3072, q[3], done) == 1024);
  CHECK(slab.alloc(1, q[4], done) == -1 && slab.live() == 4);  // full
  q[1]->consumed = true;                                       // a 512-byte hole at 256
  CHECK(slab.alloc(513, q[4], done) == -1);
  CHECK(slab.alloc(200, q[4], done) == 256);  // first fit: the hole
  CHECK(slab.alloc(256, q[5], done) == 512);
  CHECK(slab.alloc(1, q[6], done) == -1);
  q[0]->consumed = q[2]->consumed = true;
  CHECK(slab.alloc(256, q[6], done) == 0 && slab.alloc(256, q[7], done) == 768 && slab.live() == 5);
  int n = 0;
  slab.clear([&](const Req&) { n++; });
  CHECK(n == 5 && slab.live() == 0 && slab.alloc(4096, q[4], done) == 0 && slab.alloc(1, q[5], done) == -1);
}

static void test_get_count() {
  int64_t c, e;
  p2p_get_count(50, 1, &c, &e);
  CHECK(c == 50 && e == 50);
  p2p_get_count(5, 2, &c, &e);
  CHECK(c == kUndefined && e == 5);
  p2p_get_count(6, 2, &c, &e);
  CHECK(c == 3 && e == 6);
  p2p_get_count(4, 0, &c, &e);
  CHECK(c == 4 && e == kUndefined);
}

// 8 threads (ranks) post 10,000 random envelopes in all and claim as they go: every message is delivered
// exactly once, to a receive it may match, and per (src, dst, tag) in send order
static void test_threads() {
  constexpr int P = 8, N = 10000, TAGS = 3;
  Mailbox mb(P);
  // a fixed plan: message m goes src -> dst with a tag; every message has exactly one receive posted by dst
  struct Msg { int src, dst, tag; bool any_src, any_tag; };
  std::vector<Msg> plan((size_t)N);
  std::mt19937 rng(12345);
  for (auto& m : plan) {
    m.src = (int)(rng() % P);
    m.dst = (int)(rng() % P);
    m.tag = (int)(rng() % TAGS);
    // wildcards per class of receives, so that sends and receives pair up one to one whatever the interleaving:
    // every receive of rank 3 and 7 takes anything; every receive of a third of the other (dst, tag) classes
    // takes any source
    m.any_tag = m.dst % 4 == 3;
    m.any_src = m.any_tag || (m.dst * TAGS + m.tag) % 3 == 0;
  }
  std::vector<std::vector<Req>> mine((size_t)P);
  std::atomic<int> moved{0};
  std::vector<std::atomic<int>> delivered((size_t)N);
  for (auto& d : delivered) d.store(0);
  auto body = [&](int rank) {
    std::vector<std::shared_ptr<P2PPair>> got;
    for (int m = 0; m < N; m++) {
      const Msg& x = plan[(size_t)m];
      if (x.src == rank) {
        Req s = mk(true, rank, x.dst, x.tag, 8 + 4 * (m % 5));
        s->count = m;  // the message's identity
        mine[(size_t)rank].push_back(s);
        mb.post(s);
      }
      if (x.dst == rank) {
        Req r = mk(false, rank, x.any_src ? kAnySource : x.src, x.any_tag ? kAnyTag : x.tag, 64);
        mine[(size_t)rank].push_back(r);
        mb.post(r);
      }
      if (m % 7 == 0) {
        mb.claim(rank, &got);
        for (auto& p : got) delivered[(size_t)p->s->count].fetch_add(1);
        moved.fetch_add((int)got.size());
        mb.launched(got, nullptr);
      }
    }
  };
  std::vector<std::thread> th;
  for (int r = 0; r < P; r++) th.emplace_back(body, r);
  for (auto& t : th) t.join();
  std::vector<std::shared_ptr<P2PPair>> got;
  for (int r = 0; r < P; r++) {
    mb.claim(r, &got);
    for (auto& p : got) delivered[(size_t)p->s->count].fetch_add(1);
    moved.fetch_add((int)got.size());
    mb.launched(got, nullptr);
  }
  int once = 0;
  for (int m = 0; m < N; m++) once += delivered[(size_t)m].load() == 1;
  CHECK(once == N && moved.load() == N);
  for (int r = 0; r < P; r++)
    for (const Req& q : mine[(size_t)r]) {
      if (q->pair) {
        const P2PPair& p = *q->pair;
        CHECK(p.state == kPairLaunched && p.s->peer == p.r->rank);
        CHECK(p.r->tag == kAnyTag || p.s->tag == p.r->tag);
        CHECK(p.r->peer == kAnySource || p.r->peer == p.s->rank);
      } else {
        CHECK(false);  // every request was matched
      }
      mb.release(q);
    }
  CHECK(mb.pending() == 0);
}

int main() {
  test_post_order();
  test_wildcards();
  test_proc_null();
  test_non_overtaking();
  test_checks();
  test_wait_and_retire();
  test_slab();
  test_get_count();
  test_threads();
  if (g_fail) {
    printf("p2p_match_test: %d FAILED\n", g_fail);
    return 1;
  }
  printf("p2p_match_test: ok\n");
  return 0;
}
