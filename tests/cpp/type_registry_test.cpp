// type_registry_test.cpp — the derived-datatype registry (mpjexpress_amd/csrc/mpjx_strided_plan.hpp) under
// concurrent create / look-up / free from 8 threads, as rank threads use it. A stand-alone program: plain g++,
// no HIP; tests/test_strided_abi.py builds it with -fsanitize=thread where that links.
//   - every handle is >= kDerivedBase and handed out once, across all threads
//   - a live handle answers with the form it was created with, whatever the other threads do
//   - a freed handle is not found again, cannot be freed twice, and is never reissued
#include <stdio.h>

#include <atomic>
#include <set>
#include <thread>

#include "../../mpjexpress_amd/csrc/mpjx_strided_plan.hpp"

using namespace mpjx;

static std::atomic<int> failures{0};
#define EXPECT(cond)                                                    \
  do {                                                                  \
    if (!(cond)) {                                                      \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);            \
      failures++;                                                       \
    }                                                                   \
  } while (0)

constexpr int kThreads = 8, kRounds = 2000;

static void body(int tid, std::vector<int>* mine) {
  TypeRegistry& reg = TypeRegistry::get();
  TypeForm old, f, got;
  EXPECT(basic_form(8, &old));
  std::string err;
  std::vector<int> live;
  for (int k = 0; k < kRounds; k++) {
    // a form only this thread and round make: nblocks = tid + 2, blocklen = k + 1
    EXPECT(vector_form(tid + 2, k + 1, k + 1 + tid + 1, old, &f, &err) == kTypeOk);
    const int h = reg.add(f);
    EXPECT(h >= kDerivedBase);
    mine->push_back(h);
    live.push_back(h);
    EXPECT(type_form(h, &got) && got.nblocks == tid + 2 && got.blocklen == k + 1 && got.stride == k + tid + 2);
    if (k % 3 == 2) {  // free the oldest live one; it must be gone at once, the rest must stay
      const int dead = live.front();
      live.erase(live.begin());
      EXPECT(reg.release(dead));
      EXPECT(!reg.release(dead));
      EXPECT(!type_form(dead, &got));
      EXPECT(type_form(live.back(), &got) && got.nblocks == tid + 2);
    }
  }
  for (int h : live) EXPECT(type_form(h, &got) && got.nblocks == tid + 2);
}

int main() {
  std::vector<int> handles[kThreads];
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; t++) th.emplace_back(body, t, &handles[t]);
  for (std::thread& t : th) t.join();
  std::set<int> all;
  for (int t = 0; t < kThreads; t++)
    for (int h : handles[t]) EXPECT(all.insert(h).second);  // never reissued, freed or not
  EXPECT(all.size() == (size_t)kThreads * kRounds);
  EXPECT(*all.begin() == kDerivedBase && *all.rbegin() == kDerivedBase + kThreads * kRounds - 1);
  TypeForm got;
  EXPECT(!type_form(kDerivedBase + kThreads * kRounds, &got) && !type_form(kDerivedBase - 1, &got));
  EXPECT(!TypeRegistry::get().release(8) && !TypeRegistry::get().release(kDerivedBase + kThreads * kRounds));
  if (failures) {
    printf("type_registry_test: %d failures\n", failures.load());
    return 1;
  }
  printf("type_registry_test: ok\n");
  return 0;
}
