// moves_tests.cpp — the reference's block-move ccl programs (test/mpi/ccl/allgather.java, allgatherv.java,
// gatherv.java, scatterv.java, alltoall.java, alltoallv.java) written against the C++ host mirror
// (include/mpjx.hpp), run in multicore mode on GPU 0 with device arrays: the one-launch k_moves engine.
//   build: make -C mpjexpress_amd tests     run: tests/cpp/moves_tests ANS_FILE [P ...]   (default P = 4)
// ANS_FILE holds the three `ans` tables of the programs at 3 tasks (alltoallv, allgatherv, gatherv: 45
// ints each, written by tests/test_gpu_cpp_moves.py from tests/golden/ccl_moves_kat.json). The programs'
// statements give the expected buffers at any P; their first 3 blocks must equal the tables.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>

#include "mpjx.hpp"

using mpi::MPI;

static std::atomic<int> g_bad{0};
static std::vector<int> g_ans[3];  // alltoallv, allgatherv, gatherv

struct Dev {  // a device int array, filled from / read back to the host
  int* d = nullptr;
  size_t n;
  explicit Dev(const std::vector<int>& h) : n(h.size()) {
    mpi::check(hipMalloc(&d, (n ? n : 1) * sizeof(int)) == hipSuccess ? 0 : MPJX_ERR_HIP, "hipMalloc");
    (void)hipMemcpy(d, h.data(), n * sizeof(int), hipMemcpyHostToDevice);
  }
  ~Dev() { (void)hipFree(d); }
  std::vector<int> get() const {
    std::vector<int> h(n);
    (void)hipMemcpy(h.data(), d, n * sizeof(int), hipMemcpyDeviceToHost);
    return h;
  }
};

static void expect(const char* test, int rank, const std::vector<int>& got, const std::vector<int>& want) {
  for (size_t i = 0; i < want.size(); i++)
    if (got[i] != want[i]) {
      printf("%s rank %d: received data : %d at [%zu] should be : %d\n", test, rank, got[i], i, want[i]);
      g_bad++;
      return;
    }
}

static void against_table(const char* test, int rank, const std::vector<int>& got, const std::vector<int>& ans) {
  for (size_t i = 0; i < ans.size(); i++)
    if (got[i] != ans[i]) {
      printf("%s rank %d: in[%zu] = %d differs from the reference's table (%d)\n", test, rank, i, got[i], ans[i]);
      g_bad++;
      return;
    }
}

constexpr int STRIDE = 15;

static void alltoallv_test(mpi::Intracomm& c) {  // alltoallv.java
  const int tasks = c.Size(), me = c.Rank();
  std::vector<int> out(tasks * STRIDE), sdis(tasks), scount(tasks), rdis(tasks), rcount(tasks);
  for (int i = 0; i < tasks; i++) {
    sdis[i] = i * STRIDE;
    scount[i] = me == 0 ? 10 : 15;
    rdis[i] = i * 15;
    rcount[i] = i == 0 ? 10 : 15;
  }
  for (int j = 0; j < tasks; j++)
    for (int i = 0; i < STRIDE; i++) out[i + j * STRIDE] = i + me * STRIDE;
  Dev dout(out), din(std::vector<int>(tasks * STRIDE, 0));
  c.Alltoallv(dout.d, 0, scount, sdis, MPI::INT, din.d, 0, rcount, rdis, MPI::INT);
  std::vector<int> want(tasks * STRIDE, 0);
  for (int j = 0; j < tasks; j++)
    for (int i = 0; i < rcount[j]; i++) want[j * 15 + i] = i + j * STRIDE;
  const std::vector<int> in = din.get();
  expect("Alltoallv", me, in, want);
  against_table("Alltoallv", me, in, g_ans[0]);
  expect("Alltoallv sendbuf", me, dout.get(), out);
}

static void gatherv_like(mpi::Intracomm& c, bool all) {  // allgatherv.java / gatherv.java (root 0)
  const int tasks = c.Size(), me = c.Rank();
  std::vector<int> out(10), dis(tasks), rcount(tasks);
  for (int i = 0; i < 10; i++) out[i] = all ? i : 1;
  for (int i = 0; i < tasks; i++) {
    dis[i] = i * STRIDE;
    rcount[i] = i == 0 ? 10 : 5;
  }
  Dev dout(out), din(std::vector<int>(10 * STRIDE * tasks, 0));
  if (all) c.Allgatherv(dout.d, 0, me == 0 ? 10 : 5, MPI::INT, din.d, 0, rcount, dis, MPI::INT);
  else c.Gatherv(dout.d, 0, me == 0 ? 10 : 5, MPI::INT, din.d, 0, rcount, dis, MPI::INT, 0);
  std::vector<int> want(10 * STRIDE * tasks, 0);
  if (all || me == 0)
    for (int j = 0; j < tasks; j++)
      for (int i = 0; i < rcount[j]; i++) want[dis[j] + i] = out[i];
  const std::vector<int> in = din.get();
  expect(all ? "Allgatherv" : "Gatherv", me, in, want);
  if (all || me == 0) against_table(all ? "Allgatherv" : "Gatherv", me, in, g_ans[all ? 1 : 2]);
}

static void scatterv_test(mpi::Intracomm& c) {  // scatterv.java (root 0)
  const int tasks = c.Size(), me = c.Rank();
  std::vector<int> out(tasks * STRIDE), dis(tasks), scount(tasks);
  for (int i = 0; i < tasks; i++) {
    dis[i] = i * STRIDE;
    scount[i] = i == 0 ? 10 : 5;
  }
  for (int i = 0; i < tasks * STRIDE; i++) out[i] = i;
  Dev dout(out), din(std::vector<int>(10, 0));
  c.Scatterv(dout.d, 0, scount, dis, MPI::INT, din.d, 0, scount[me], MPI::INT, 0);
  std::vector<int> want(10, 0);
  for (int i = 0; i < scount[me]; i++) want[i] = dis[me] + i;
  expect("Scatterv", me, din.get(), want);
}

static void equal_test(mpi::Intracomm& c, bool all2all) {  // allgather.java / alltoall.java
  const int tasks = c.Size(), me = c.Rank();
  constexpr int MAXLEN = 10000;
  Dev dout(std::vector<int>((size_t)MAXLEN * (all2all ? tasks : 1), me)), din(std::vector<int>((size_t)MAXLEN * tasks, -1));
  for (int j = 1; j <= MAXLEN; j *= 10) {
    if (all2all) c.Alltoall(dout.d, 0, j, MPI::INT, din.d, 0, j, MPI::INT);
    else c.Allgather(dout.d, 0, j, MPI::INT, din.d, 0, j, MPI::INT);
    const std::vector<int> in = din.get();
    for (int i = 0; i < tasks; i++)
      for (int k = 0; k < j; k++)
        if (in[k + i * j] != i) {
          printf("%s rank %d: bad answer (%d) at index %d of %d (should be %d)\n", all2all ? "Alltoall" : "Allgather", me,
                 in[k + i * j], k + i * j, j * tasks, i);
          g_bad++;
          i = tasks;
          break;
        }
  }
}

static void run_world(int P, const std::function<void(mpi::Intracomm&)>& fn) {
  std::vector<mpi::Intracomm> world = mpi::smp_world(P, std::vector<int>(P, 0));
  std::vector<std::thread> th;
  for (int r = 0; r < P; r++)
    th.emplace_back([&, r] {
      (void)hipSetDevice(0);
      try {
        fn(world[r]);
      } catch (const mpi::MPIException& e) {
        printf("rank %d: MPIException: %s\n", r, e.what());
        g_bad++;
      }
    });
  for (auto& t : th) t.join();
}

int main(int argc, char** argv) {
  if (argc < 2) {
    printf("usage: moves_tests ANS_FILE [P ...]\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    printf("cannot read %s\n", argv[1]);
    return 2;
  }
  for (auto& a : g_ans) {
    a.resize(45);
    for (int& x : a)
      if (fscanf(f, "%d", &x) != 1) {
        printf("%s: expected 3 x 45 integers\n", argv[1]);
        return 2;
      }
  }
  fclose(f);
  std::vector<int> Ps;
  for (int i = 2; i < argc; i++) Ps.push_back(atoi(argv[i]));
  if (Ps.empty()) Ps.push_back(4);
  for (int P : Ps) {
    if (P < 3) {
      printf("P = %d: the tables hold 3 tasks' blocks\n", P);
      return 2;
    }
    run_world(P, alltoallv_test);
    run_world(P, [](mpi::Intracomm& c) { gatherv_like(c, true); });
    run_world(P, [](mpi::Intracomm& c) { gatherv_like(c, false); });
    run_world(P, scatterv_test);
    run_world(P, [](mpi::Intracomm& c) { equal_test(c, false); });
    run_world(P, [](mpi::Intracomm& c) { equal_test(c, true); });
    printf("P=%d: Allgather Allgatherv Gatherv Scatterv Alltoall Alltoallv TEST COMPLETE\n", P);
  }
  // differing datatypes throw before anything is enqueued
  bool threw = false;
  run_world(1, [&](mpi::Intracomm& c) {
    Dev a(std::vector<int>(4, 0)), b(std::vector<int>(4, 0));
    try {
      c.Allgather(a.d, 0, 4, MPI::INT, b.d, 0, 4, MPI::FLOAT);
    } catch (const mpi::MPIException&) {
      threw = true;
    }
  });
  if (!threw) {
    printf("Allgather with differing datatypes did not throw\n");
    g_bad++;
  }
  printf("%s (%d bad)\n", g_bad ? "FAILED" : "ALL MOVES TESTS PASSED", g_bad.load());
  return g_bad ? 1 : 0;
}
