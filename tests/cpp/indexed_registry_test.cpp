// indexed_registry_test.cpp — the datatype registry with the irregular forms (Hvector / Indexed / Hindexed,
// mpjexpress_amd/csrc/mpjx_indexed_plan.hpp) under concurrent create / look-up / free from 8 threads, as rank
// threads use it. A stand-alone program: plain g++, no HIP; tests/test_indexed_abi.py builds it with
// -fsanitize=thread where that links.
//   - a live handle answers with the block list it was created with, whatever the other threads do
//   - a form looked up before its handle is freed keeps its block list (a call in flight holds the layout)
//   - a new type over an oldtype that another thread frees meanwhile is either built whole or refused
#include <stdio.h>

#include <atomic>
#include <thread>

#include "../../mpjexpress_amd/csrc/mpjx_indexed_plan.hpp"

using namespace mpjx;

static std::atomic<int> failures{0};
#define EXPECT(cond)                                         \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      failures++;                                            \
    }                                                        \
  } while (0)

constexpr int kThreads = 8, kRounds = 1500;
static std::atomic<int> shared_old{0};  // a handle any thread may build on or free

static void body(int tid) {
  TypeRegistry& reg = TypeRegistry::get();
  TypeForm old, f, got, held;
  EXPECT(basic_form(5, &old));
  std::string err;
  std::vector<int> live;
  for (int k = 0; k < kRounds; k++) {
    // blocks only this thread and round make: (k + 2, tid + 1) then (0, 1)
    const int64_t bl[2] = {tid + 1, 1}, d[2] = {k + 2 + tid, 0};
    EXPECT(((k & 1) ? indexed_form : hindexed_form)(2, bl, d, old, &f, &err) == kTypeOk && f.irr);
    const int h = reg.add(f);
    live.push_back(h);
    EXPECT(type_form(h, &got) && got.irr && got.code == h && got.size() == tid + 2 && got.irr->tab[0].off == 4 * (k + 2 + tid));
    if (k % 3 == 2) {
      const int dead = live.front();
      live.erase(live.begin());
      EXPECT(type_form(dead, &held) && held.irr);
      EXPECT(reg.release(dead) && !reg.release(dead) && !type_form(dead, &got));
      EXPECT(held.irr->tab.size() == 2 && held.size() == tid + 2);  // the copy owns its layout
    }
    if (k % 5 == 0) {  // publish one, build on whatever is published, free what was there before
      const int mine = reg.add(f), was = shared_old.exchange(mine);
      TypeForm base, over;
      if (was && type_form(was, &base)) {
        const int rc = hvector_form(2, 1, 4096, base, &over, &err);
        EXPECT(rc == kTypeOk && over.size() == 2 * base.size());
      }
      if (was) (void)reg.release(was);
    }
  }
  for (int h : live) EXPECT(type_form(h, &got) && got.size() == tid + 2);
}

int main() {
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; t++) th.emplace_back(body, t);
  for (std::thread& t : th) t.join();
  if (failures) {
    printf("indexed_registry_test: %d failures\n", failures.load());
    return 1;
  }
  printf("indexed_registry_test: ok\n");
  return 0;
}
