// bench_preq.cpp — the rows of tools/bench_preq.py from C++ rank threads (no interpreter lock): the P = 4 halo
// exchange on 1024 x 1024 DOUBLE tiles through Isend / Irecv / Waitall every iteration, through persistent
// requests (Startall / Waitall) with the device segment pool, and the same with MPJX_P2P_POOL=0; and 26 messages
// of 8 KiB per rank (message k to rank (me + 1 + k % 3) % 4 under tag k), persistent, pool on and off.
// Host wall-clock per exchange on rank 0, median / min / max of --iters (default 30) after 5 warm-up exchanges, on
// cold operands: before every timed exchange rank 0 rewrites a 512 MiB buffer and the ranks meet at a barrier.
//   build: make -C mpjexpress_amd tools     run: tools/bench_preq_cpp [iters]     one JSON line per row
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#include "mpjx.hpp"

using mpi::MPI;

static int g_iters = 30;
constexpr int kWarmup = 5;
constexpr size_t kFlushBytes = (size_t)512 << 20;
static void* g_flush = nullptr;

struct Row {
  double med = 0, lo = 0, hi = 0;
  long long launches = 0, pool_launches = 0, puts = 0, hits = 0;
};

static void timed(mpi::Intracomm& c, const std::function<void()>& step, Row* out) {
  std::vector<double> ts;
  for (int i = 0; i < kWarmup + g_iters; i++) {
    if (c.Rank() == 0) {
      (void)hipMemset(g_flush, i & 0xff, kFlushBytes);
      (void)hipDeviceSynchronize();
    }
    c.Barrier();
    const auto t0 = std::chrono::steady_clock::now();
    step();
    const auto t1 = std::chrono::steady_clock::now();
    if (i >= kWarmup) ts.push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
  }
  std::sort(ts.begin(), ts.end());
  out->med = ts.size() % 2 ? ts[ts.size() / 2] : 0.5 * (ts[ts.size() / 2 - 1] + ts[ts.size() / 2]);
  out->lo = ts.front();
  out->hi = ts.back();
}

static void counters(mpi::Intracomm& c, Row* out) {
  int64_t l = 0, pl = 0, pu = 0, hi = 0;
  mpi::check(mpjx_comm_p2p_stats(c.handle(), &l, nullptr, nullptr, nullptr), "mpjx_comm_p2p_stats");
  mpi::check(mpjx_comm_p2p_pool_stats(c.handle(), &pl, &pu, &hi, nullptr, nullptr), "mpjx_comm_p2p_pool_stats");
  out->launches = l, out->pool_launches = pl, out->puts = pu, out->hits = hi;
}

static void halo(mpi::Intracomm& c, bool persistent, Row* out) {
  constexpr int T = 1024, N = T + 2;
  const int me = c.Rank(), i = me / 2, j = me % 2;
  const int north = ((i + 1) % 2) * 2 + j, south = north, west = i * 2 + (j + 1) % 2, east = west;
  mpi::Datatype col = mpi::Datatype::Vector(T, 1, N, MPI::DOUBLE);
  double* t = nullptr;
  mpi::check(hipMalloc(&t, sizeof(double) * N * N) == hipSuccess ? 0 : MPJX_ERR_HIP, "hipMalloc");
  (void)hipMemset(t, me + 1, sizeof(double) * N * N);
  std::vector<mpi::Prequest> preq;
  if (persistent) {
    preq.push_back(c.Recv_init(t, (N - 1) * N + 1, T, MPI::DOUBLE, south, 0));
    preq.push_back(c.Recv_init(t, 1, T, MPI::DOUBLE, north, 1));
    preq.push_back(c.Recv_init(t, N + N - 1, 1, col, east, 2));
    preq.push_back(c.Recv_init(t, N, 1, col, west, 3));
    preq.push_back(c.Send_init(t, N + 1, T, MPI::DOUBLE, north, 0));
    preq.push_back(c.Send_init(t, (N - 2) * N + 1, T, MPI::DOUBLE, south, 1));
    preq.push_back(c.Send_init(t, N + 1, 1, col, west, 2));
    preq.push_back(c.Send_init(t, N + N - 2, 1, col, east, 3));
  }
  timed(c, [&] {
    if (persistent) {
      mpi::Prequest::Startall(preq);
      mpi::Request::Waitall(preq);
      return;
    }
    std::vector<mpi::Request> req;
    req.push_back(c.Irecv(t, (N - 1) * N + 1, T, MPI::DOUBLE, south, 0));
    req.push_back(c.Irecv(t, 1, T, MPI::DOUBLE, north, 1));
    req.push_back(c.Irecv(t, N + N - 1, 1, col, east, 2));
    req.push_back(c.Irecv(t, N, 1, col, west, 3));
    req.push_back(c.Isend(t, N + 1, T, MPI::DOUBLE, north, 0));
    req.push_back(c.Isend(t, (N - 2) * N + 1, T, MPI::DOUBLE, south, 1));
    req.push_back(c.Isend(t, N + 1, 1, col, west, 2));
    req.push_back(c.Isend(t, N + N - 2, 1, col, east, 3));
    mpi::Request::Waitall(req);
  }, out);
  counters(c, out);
  c.Barrier();
  preq.clear();
  col.Free();
  (void)hipFree(t);
}

static void neighbours(mpi::Intracomm& c, Row* out) {
  constexpr int K = 26, n = 8192 / 8;
  const int me = c.Rank();
  double *s = nullptr, *r = nullptr;
  mpi::check(hipMalloc(&s, sizeof(double) * K * n) == hipSuccess ? 0 : MPJX_ERR_HIP, "hipMalloc");
  mpi::check(hipMalloc(&r, sizeof(double) * K * n) == hipSuccess ? 0 : MPJX_ERR_HIP, "hipMalloc");
  (void)hipMemset(s, me + 1, sizeof(double) * K * n);
  std::vector<mpi::Prequest> preq;
  for (int k = 0; k < K; k++) preq.push_back(c.Recv_init(r, k * n, n, MPI::DOUBLE, ((me - 1 - k % 3) % 4 + 4) % 4, k));
  for (int k = 0; k < K; k++) preq.push_back(c.Send_init(s, k * n, n, MPI::DOUBLE, (me + 1 + k % 3) % 4, k));
  timed(c, [&] {
    mpi::Prequest::Startall(preq);
    mpi::Request::Waitall(preq);
  }, out);
  counters(c, out);
  c.Barrier();
  preq.clear();
  (void)hipFree(s);
  (void)hipFree(r);
}

static void run_row(const char* bench, const char* mode, bool pool, const std::function<void(mpi::Intracomm&, Row*)>& fn) {
  if (pool) unsetenv("MPJX_P2P_POOL");
  else setenv("MPJX_P2P_POOL", "0", 1);  // read once, when the world is created
  std::vector<mpi::Intracomm> world = mpi::smp_world(4, std::vector<int>(4, 0));
  unsetenv("MPJX_P2P_POOL");
  std::vector<Row> rows(4);
  std::vector<std::thread> th;
  for (int r = 0; r < 4; r++)
    th.emplace_back([&, r] {
      try {
        (void)hipSetDevice(0);
        world[(size_t)r].SetP2PTimeout(30);
        fn(world[(size_t)r], &rows[(size_t)r]);
      } catch (const std::exception& e) {
        printf("rank %d: %s\n", r, e.what());
        exit(1);
      }
    });
  for (auto& t : th) t.join();
  Row sum = rows[0];
  for (int r = 1; r < 4; r++)
    sum.launches += rows[(size_t)r].launches, sum.pool_launches += rows[(size_t)r].pool_launches, sum.puts += rows[(size_t)r].puts,
        sum.hits += rows[(size_t)r].hits;
  printf("{\"bench\": \"%s\", \"host\": \"c++\", \"mode\": \"%s\", \"us\": %.2f, \"us_min\": %.2f, \"us_max\": %.2f, "
         "\"launches_all_ranks\": %lld, \"pool_launches_all_ranks\": %lld, \"puts_all_ranks\": %lld, \"hits_all_ranks\": %lld}\n",
         bench, mode, sum.med, sum.lo, sum.hi, sum.launches, sum.pool_launches, sum.puts, sum.hits);
  fflush(stdout);
}

int main(int argc, char** argv) {
  if (argc > 1) g_iters = std::max(1, atoi(argv[1]));
  (void)hipSetDevice(0);
  if (hipMalloc(&g_flush, kFlushBytes) != hipSuccess) {
    printf("hipMalloc of the flush buffer failed\n");
    return 1;
  }
  using namespace std::placeholders;
  run_row("halo", "isend", true, [](mpi::Intracomm& c, Row* o) { halo(c, false, o); });
  run_row("halo", "persistent", true, [](mpi::Intracomm& c, Row* o) { halo(c, true, o); });
  run_row("halo", "persistent_pool_off", false, [](mpi::Intracomm& c, Row* o) { halo(c, true, o); });
  run_row("neighbours26", "persistent", true, neighbours);
  run_row("neighbours26", "persistent_pool_off", false, neighbours);
  (void)hipFree(g_flush);
  return 0;
}
