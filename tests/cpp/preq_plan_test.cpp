// CPU test of the persistent requests' host side (mpjexpress_amd/csrc/mpjx_p2p_plan.hpp: Persist, Mailbox::post_all;
// mpjx_msgs_pool_plan.hpp: PoolMap): plain C++17, no HIP. Built by the Makefile with g++, and by
// tests/test_preq_abi.py under -fsanitize=address,undefined and -fsanitize=thread.
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <thread>

#include "../../mpjexpress_amd/csrc/mpjx_msgs_pool_plan.hpp"
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

static P2PReq plan(bool send, int rank, int peer, int tag, int64_t bytes = 8, int base = 5, uint64_t addr = 0) {
  P2PReq q;
  q.send = send;
  q.rank = rank;
  q.peer = peer;
  q.tag = tag;
  q.base = base;
  q.bsz = 4;
  q.bytes = bytes;
  q.lay = run(addr ? addr : (uint64_t)(0x10000 + 0x1000 * rank + (send ? 0 : 0x800)), bytes);
  return q;
}

static Mailbox::Clock::time_point soon() { return Mailbox::Clock::now() + std::chrono::seconds(60); }

// What a wait does with the mailbox alone: claim and "move" whatever has matched, until q is settled
static void wait_one(Mailbox& mb, int rank, const Req& q) {
  for (;;) {
    std::vector<std::shared_ptr<P2PPair>> batch;
    mb.claim(rank, &batch);
    if (!batch.empty()) mb.launched(batch, nullptr);
    const Mailbox::Wake w = mb.wait(q, soon(), nullptr);
    if (w == Mailbox::kWakeMatched) continue;
    CHECK(w == Mailbox::kWakeSettled);
    return;
  }
}

static void test_serials_and_plan() {
  Persist a(plan(true, 0, 1, 3)), b(plan(false, 1, 0, 3));
  CHECK(a.serial() != 0 && b.serial() != 0 && a.serial() != b.serial());
  CHECK(!a.active() && !a.plan.pair && !a.plan.ready && a.plan.freed && !a.plan.freed->load());
  Req x = a.start();
  CHECK(x && a.active() && x->serial == a.serial() && x->freed == a.plan.freed && x.get() != &a.plan);
  CHECK(!a.start());  // active: a second start gives nothing to post
  a.finish(nullptr);
  CHECK(!a.active());
  Req y = a.start();
  CHECK(y && y != x && y->serial == a.serial());  // a fresh request at every start, the same serial
  a.finish(nullptr);
  // a plain request carries 0
  CHECK(plan(true, 0, 1, 3).serial == 0);
  std::shared_ptr<std::atomic<bool>> flag;
  {
    Persist c(plan(true, 0, 1, 4));
    flag = c.plan.freed;
    CHECK(c.serial() > b.serial());
  }
  CHECK(flag->load());  // freed
}

// inactive -> active -> inactive, 1,000 rounds from 8 rank threads: each sends to its right neighbour and receives
// from its left one through two persistent requests, started with post_all
static void test_lifecycle_threads() {
  constexpr int P = 8, kRounds = 1000;
  Mailbox mb(P);
  std::vector<std::thread> th;
  for (int me = 0; me < P; me++)
    th.emplace_back([&mb, me] {
      const int right = (me + 1) % P, left = (me + P - 1) % P;
      Persist s(plan(true, me, right, 11, 16)), r(plan(false, me, left, 11, 16));
      for (int it = 0; it < kRounds; it++) {
        CHECK(!s.active() && !r.active());
        Req qs = s.start(), qr = r.start();
        CHECK(qs && qr && qs->serial == s.serial() && !qs->pair);
        mb.post_all({qr, qs});
        CHECK(s.active() && r.active());
        wait_one(mb, me, qr);
        wait_one(mb, me, qs);
        const P2PStatus st = p2p_status(*qr);
        CHECK(st.source == left && st.tag == 11 && st.bytes == 16 && st.error == kP2POk);
        CHECK(qr->pair && qr->pair->s->serial != 0 && qr->pair->r->serial == r.serial());
        s.finish(&mb);
        r.finish(&mb);
        CHECK(!s.active() && !r.active() && !qs->pair && !qr->pair);
      }
    });
  for (auto& t : th) t.join();
  CHECK(mb.pending() == 0);
}

// Startall posts in array order under one lock: two sends of one (source, dest, tag) meet two receives in order
static void test_array_order() {
  Mailbox mb(2);
  Persist s1(plan(true, 0, 1, 5, 8)), s2(plan(true, 0, 1, 5, 16)), r1(plan(false, 1, 0, 5, 16)), r2(plan(false, 1, 0, 5, 16));
  for (int it = 0; it < 3; it++) {
    Req a = s1.start(), b = s2.start(), x = r1.start(), y = r2.start();
    if (it % 2 == 0) {
      CHECK(mb.post_all({a, b}) == 0);
      CHECK(mb.post_all({x, y}) == 2);
    } else {
      CHECK(mb.post_all({x, y}) == 0);
      CHECK(mb.post_all({a, b}) == 2);
    }
    CHECK(x->pair && x->pair->s == a && y->pair && y->pair->s == b);
    CHECK(p2p_status(*x).bytes == 8 && p2p_status(*y).bytes == 16);
    wait_one(mb, 1, x);
    wait_one(mb, 1, y);
    for (Persist* p : {&s1, &s2, &r1, &r2}) p->finish(&mb);
  }
  // a mixed list: a PROC_NULL entry completes at once and does not disturb the order
  Persist n(plan(true, 0, kProcNull, 5, 8));
  Req a = s1.start(), z = n.start(), b = s2.start();
  CHECK(mb.post_all({a, z, b}) == 0 && z->null_peer && mb.pending() == 2);
  CHECK(mb.wait(z, soon(), nullptr) == Mailbox::kWakeSettled);
  Req x = r1.start();
  CHECK(mb.post(x) && x->pair->s == a);
  for (Persist* p : {&s1, &s2, &r1, &n}) p->finish(&mb);
  CHECK(mb.pending() == 0);
}

static void test_free_while_active() {
  Mailbox mb(2);
  {  // unmatched: the activation is withdrawn
    Persist s(plan(true, 0, 1, 1));
    Req q = s.start();
    mb.post(q);
    CHECK(mb.pending() == 1);
    s.finish(&mb);
    CHECK(mb.pending() == 0 && q->orphan && !s.active());
    // the receive that comes later does not match the withdrawn send
    Persist r(plan(false, 1, 0, 1));
    Req x = r.start();
    CHECK(!mb.post(x) && mb.pending() == 1);
    r.finish(&mb);
  }
  {  // matched, not yet moved: the pair is let go by this side; the peer still completes
    Persist s(plan(true, 0, 1, 2)), r(plan(false, 1, 0, 2));
    Req q = s.start(), x = r.start();
    mb.post(q);
    CHECK(mb.post(x));
    s.finish(&mb);
    CHECK(!q->pair && x->pair);
    wait_one(mb, 1, x);
    CHECK(p2p_status(*x).source == 0 && p2p_status(*x).error == kP2POk);
    r.finish(&mb);
    // both can be started again
    Req q2 = s.start(), x2 = r.start();
    CHECK(q2 && x2);
    mb.post_all({q2, x2});
    wait_one(mb, 0, q2);
    s.finish(&mb);
    r.finish(&mb);
  }
  {  // a base-type mismatch fails both activations at match; both requests are startable again
    Persist s(plan(true, 0, 1, 3, 8, 5)), r(plan(false, 1, 0, 3, 8, 8));
    Req q = s.start(), x = r.start();
    mb.post_all({q, x});
    CHECK(q->pair && q->pair->state == kPairFailed && p2p_status(*x).error == kP2PErrArg);
    s.finish(&mb);
    r.finish(&mb);
    CHECK(s.start() && r.start());
    s.finish(nullptr);
    r.finish(nullptr);
  }
  CHECK(mb.pending() == 0);
}

static void test_pool_map() {
  const MsgSeg seg = msg_bytes_seg(0x100000, 0x900000, 4096);
  PoolMap pm(4);
  CHECK(pm.capacity() == 4 && pm.in_use() == 0 && !pm.find(1, 2));
  std::vector<std::unique_ptr<Persist>> s, r;
  for (int i = 0; i < 6; i++) {
    s.emplace_back(new Persist(plan(true, 0, 1, i)));
    r.emplace_back(new Persist(plan(false, 1, 0, i)));
  }
  auto put = [&](int i, int j) { return pm.put(s[i]->serial(), r[j]->serial(), seg, s[i]->plan.freed, r[j]->plan.freed); };
  std::set<int> slots;
  for (int i = 0; i < 4; i++) {
    const int sl = put(i, i);
    CHECK(sl >= 0 && sl < 4 && slots.insert(sl).second);
    const PoolMap::Entry* e = pm.find(s[i]->serial(), r[i]->serial());
    CHECK(e && e->slot == sl && e->bytes == 4096);
    CHECK(e && e->tiles == (uint32_t)msg_tiles(seg, kStridedTile) && e->tiles_nt == (uint32_t)msg_tiles(seg, kStridedTileNT));
  }
  CHECK(pm.in_use() == 4);
  CHECK(put(0, 0) == -1);             // already there
  CHECK(!pm.find(s[0]->serial(), r[1]->serial()));  // the key is the PAIR
  CHECK(put(4, 4) == -1 && pm.in_use() == 4);       // full of live pairs
  CHECK(!pm.find(s[4]->serial(), r[4]->serial()));
  // freeing one request of a pair makes its slot reclaimable; the pair is never looked up again because the
  // request that replaces it has a new serial
  const uint64_t dead = r[1]->serial();
  const int was = pm.find(s[1]->serial(), dead)->slot;
  r[1].reset(new Persist(plan(false, 1, 0, 1)));
  CHECK(r[1]->serial() != dead && !pm.find(s[1]->serial(), r[1]->serial()));
  const int sl = put(1, 1);
  CHECK(sl == was && pm.in_use() == 4);  // the dead pair's slot, reclaimed at this put
  CHECK(!pm.find(s[1]->serial(), dead));
  CHECK(put(5, 5) == -1);
  s[0].reset();
  s[2].reset();
  CHECK(pm.reclaim() == 2 && pm.in_use() == 2);
  CHECK(put(4, 4) >= 0 && put(5, 5) >= 0 && pm.in_use() == 4);
  // a put whose store could not be enqueued is undone: no lookup finds it and its slot is free again
  const int had = pm.find(s[5]->serial(), r[5]->serial())->slot;
  pm.erase(s[5]->serial(), r[5]->serial());
  pm.erase(s[5]->serial(), r[5]->serial());  // twice is harmless
  CHECK(!pm.find(s[5]->serial(), r[5]->serial()) && pm.in_use() == 3);
  CHECK(put(5, 5) == had && pm.in_use() == 4);
  // what cannot be pooled: an empty segment, one of more tiles than a launch takes
  PoolMap big;
  CHECK(big.capacity() == kPoolSlots);
  CHECK(big.put(1, 2, msg_bytes_seg(0x1000, 0x2000, 0), nullptr, nullptr) == -1);
  CHECK(big.put(1, 2, seg, nullptr, nullptr, 0) == -1 && big.in_use() == 0);
  CHECK(big.put(1, 2, seg, nullptr, nullptr) == 0 && big.in_use() == 1);
}

int main() {
  test_serials_and_plan();
  test_lifecycle_threads();
  test_array_order();
  test_free_while_active();
  test_pool_map();
  if (g_fail) {
    printf("preq_plan_test: %d FAILED\n", g_fail.load());
    return 1;
  }
  printf("preq_plan_test: ok\n");
  return 0;
}
