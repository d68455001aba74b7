// preq_tests.cpp — persistent requests (Send_init / Recv_init, Prequest::Start / Startall) written against the
// C++ host mirror (include/mpjx.hpp), run in multicore mode on GPU 0 with device arrays and one thread per rank:
//   reuse   P = 2, 4 iterations: the send buffer is rewritten between iterations and the receiver sees the new
//           values; the requests stay non-null and inactive after each wait
//   halo    the 2 x 2 periodic halo of p2p_tests.cpp (rows contiguous, columns Datatype::Vector) with the
//           requests made once, then 4 x (Startall, Waitall), the interior changed between iterations
//   pool    30 persistent pairs of 8 B waited on by one rank, the peer's starts made first: iteration 1 takes two
//           k_msgs launches and stores 30 segments; iterations 2 and 3 take ONE k_msgs_pool launch each. The same
//           with 513 pairs: 22 k_msgs launches, then TWO k_msgs_pool launches
// Left to tests/test_gpu_preq.py, which runs them from Python rank threads: the halo's Indexed layout, its
// comparison with the same exchange through Isend / Irecv (here the tile is compared with a computed expectation),
// and its reruns under MPJX_P2P_POOL=0 and MPJX_P2P_BATCH=0.
//   build: make -C mpjexpress_amd tests     run: tests/cpp/preq_tests
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

template <class T>
struct Dev {  // a device array, filled from / read back to the host
  T* d = nullptr;
  size_t n;
  explicit Dev(const std::vector<T>& h) : n(h.size()) {
    mpi::check(hipMalloc(&d, (n ? n : 1) * sizeof(T)) == hipSuccess ? 0 : MPJX_ERR_HIP, "hipMalloc");
    put(h);
  }
  ~Dev() { (void)hipFree(d); }
  void put(const std::vector<T>& h) { (void)hipMemcpy(d, h.data(), n * sizeof(T), hipMemcpyHostToDevice); }
  std::vector<T> get() const {
    std::vector<T> h(n);
    (void)hipMemcpy(h.data(), d, n * sizeof(T), hipMemcpyDeviceToHost);
    return h;
  }
};

static void bad(const char* test, int rank, const char* what, long got, long want) {
  printf("%s rank %d: %s = %ld should be %ld\n", test, rank, what, got, want);
  g_bad++;
}

static void idle(const char* test, int me, std::vector<mpi::Prequest>& req) {
  for (mpi::Prequest& r : req)
    if (r.Is_null() || r.Is_active()) bad(test, me, "request null or active after Waitall", 1, 0);
}

static void reuse_test(mpi::Intracomm& c) {
  const int me = c.Rank(), other = 1 - me, n = 900;
  Dev<int> s(std::vector<int>(1000, 0)), r(std::vector<int>(1000, -1));
  std::vector<mpi::Prequest> req;
  req.push_back(c.Recv_init(r.d, 5, n, MPI::INT, other, 4));
  req.push_back(c.Send_init(s.d, 3, n, MPI::INT, other, 4));
  for (int it = 0; it < 4; it++) {
    std::vector<int> h(1000);
    for (int i = 0; i < 1000; i++) h[(size_t)i] = i * (it + 1) + 100000 * me;
    s.put(h);
    mpi::Prequest::Startall(req);
    if (!req[0].Is_active()) bad("reuse", me, "active after Startall", 0, 1);
    const std::vector<mpi::Status> st = mpi::Request::Waitall(req);
    idle("reuse", me, req);
    if (st[0].source != other || st[0].tag != 4 || st[0].Get_count(MPI::INT) != n) bad("reuse", me, "recv status", st[0].source, other);
    if (st[1].source != MPI::PROC_NULL || st[1].Get_count(MPI::INT) != 0) bad("reuse", me, "send status not empty", st[1].source, MPI::PROC_NULL);
    const mpi::Status again = req[0].Wait();  // inactive: returns at once with the empty status
    if (again.source != MPI::PROC_NULL || again.tag != MPI::ANY_TAG) bad("reuse", me, "wait on inactive", again.source, MPI::PROC_NULL);
    const std::vector<int> got = r.get();
    for (int i = 0; i < 1000; i++) {
      const int want = (i >= 5 && i < 5 + n) ? (i - 2) * (it + 1) + 100000 * other : -1;
      if (got[(size_t)i] != want) {
        bad("reuse", me, "recvbuf[i]", got[(size_t)i], want);
        break;
      }
    }
    c.Barrier();
  }
}

constexpr int N = 34, kIters = 4;
static std::vector<double> tile_of(int rank, int bumps) {
  std::vector<double> t((size_t)N * N);
  for (int i = 0; i < N * N; i++) t[(size_t)i] = rank * 10000.0 + i;
  for (int r = 1; r < N - 1; r++)
    for (int k = 1; k < N - 1; k++) t[(size_t)(r * N + k)] += 0.5 * (rank + 1) * bumps;
  return t;
}

static void halo_test(mpi::Intracomm& c) {
  const int me = c.Rank(), i = me / 2, j = me % 2;
  const int north = ((i + 1) % 2) * 2 + j, south = north, west = i * 2 + (j + 1) % 2, east = west;
  mpi::Datatype col = mpi::Datatype::Vector(N - 2, 1, N, MPI::DOUBLE);
  std::vector<double> mine = tile_of(me, 0);
  Dev<double> t(mine);
  std::vector<mpi::Prequest> req;
  req.push_back(c.Recv_init(t.d, (N - 1) * N + 1, N - 2, MPI::DOUBLE, south, 0));
  req.push_back(c.Recv_init(t.d, 1, N - 2, MPI::DOUBLE, north, 1));
  req.push_back(c.Recv_init(t.d, N + N - 1, 1, col, east, 2));
  req.push_back(c.Recv_init(t.d, N, 1, col, west, 3));
  req.push_back(c.Send_init(t.d, N + 1, N - 2, MPI::DOUBLE, north, 0));
  req.push_back(c.Send_init(t.d, (N - 2) * N + 1, N - 2, MPI::DOUBLE, south, 1));
  req.push_back(c.Send_init(t.d, N + 1, 1, col, west, 2));
  req.push_back(c.Send_init(t.d, N + N - 2, 1, col, east, 3));
  for (int it = 0; it < kIters; it++) {
    mpi::Prequest::Startall(req);
    const std::vector<mpi::Status> st = mpi::Request::Waitall(req);
    idle("halo", me, req);
    for (int k = 0; k < 4; k++) {
      if (st[(size_t)k].tag != k) bad("halo", me, "status.tag", st[(size_t)k].tag, k);
      if (st[(size_t)k].Get_count(MPI::DOUBLE) != N - 2) bad("halo", me, "Get_count", st[(size_t)k].Get_count(MPI::DOUBLE), N - 2);
    }
    // the halo ring holds the neighbours' interiors as of this iteration; the interior is this rank's own
    std::vector<double> want = tile_of(me, it);
    const std::vector<double> s = tile_of(south, it), n = tile_of(north, it), e = tile_of(east, it), w = tile_of(west, it);
    for (int k = 1; k < N - 1; k++) {
      want[(size_t)((N - 1) * N + k)] = s[(size_t)(N + k)];
      want[(size_t)k] = n[(size_t)((N - 2) * N + k)];
      want[(size_t)(k * N + N - 1)] = e[(size_t)(k * N + 1)];
      want[(size_t)(k * N)] = w[(size_t)(k * N + N - 2)];
    }
    std::vector<double> got = t.get();
    for (int k = 0; k < N * N; k++)
      if (got[(size_t)k] != want[(size_t)k]) {
        bad("halo", me, "tile element", (long)got[(size_t)k], (long)want[(size_t)k]);
        printf("  iteration %d element %d\n", it, k);
        break;
      }
    // the next iteration sends a changed interior (the ring stays as received)
    for (int r = 1; r < N - 1; r++)
      for (int k = 1; k < N - 1; k++) got[(size_t)(r * N + k)] += 0.5 * (me + 1);
    t.put(got);
  }
  c.Barrier();
  req.clear();
  col.Free();
}

struct PoolStats {
  int64_t launches = 0, pool_launches = 0, puts = 0, hits = 0, used = 0;
};
static PoolStats stats_of(mpi::Intracomm& c) {
  PoolStats p;
  int tmax = 0, bmax = 0;
  mpi::check(mpjx_comm_p2p_stats(c.handle(), &p.launches, nullptr, nullptr, &tmax), "mpjx_comm_p2p_stats");
  mpi::check(mpjx_comm_p2p_pool_stats(c.handle(), &p.pool_launches, &p.puts, &p.hits, &p.used, &bmax), "mpjx_comm_p2p_pool_stats");
  if (tmax != 24 || bmax != 512) bad("pool", c.Rank(), "table_max / batch_max", tmax, 24);
  return p;
}

static void pool_test(mpi::Intracomm& c, int kPairs, int table_launches, int pool_launches) {
  const int me = c.Rank(), other = 1 - me;
  Dev<int> s(std::vector<int>((size_t)kPairs * 4, 0)), r(std::vector<int>((size_t)kPairs * 4, -1));
  std::vector<mpi::Prequest> req;
  for (int k = 0; k < kPairs; k++)  // message k goes 0 -> 1 for even k, 1 -> 0 for odd k
    if (k % 2 == me) req.push_back(c.Send_init(s.d, 4 * k + 1, 2, MPI::INT, other, k));
    else req.push_back(c.Recv_init(r.d, 4 * k + 1, 2, MPI::INT, other, k));
  for (int it = 0; it < 3; it++) {
    std::vector<int> h((size_t)kPairs * 4);
    for (int i = 0; i < kPairs * 4; i++) h[(size_t)i] = i + 1000 * me + 7 * it;
    s.put(h);
    r.put(std::vector<int>((size_t)kPairs * 4, -1));
    const PoolStats b = stats_of(c);
    // rank 1 starts, Barrier, rank 0 starts and waits (claiming every pair), Barrier, rank 1 waits
    if (me == 1) mpi::Prequest::Startall(req);
    c.Barrier();
    if (me == 0) {
      mpi::Prequest::Startall(req);
      mpi::Request::Waitall(req);
    }
    c.Barrier();
    if (me == 1) mpi::Request::Waitall(req);
    c.Barrier();
    const PoolStats a = stats_of(c);
    const long want[4] = {me == 0 ? (it == 0 ? table_launches : pool_launches) : 0, me == 0 && it > 0 ? pool_launches : 0,
                          me == 0 && it == 0 ? kPairs : 0, me == 0 && it > 0 ? kPairs : 0};
    const long got[4] = {(long)(a.launches - b.launches), (long)(a.pool_launches - b.pool_launches), (long)(a.puts - b.puts),
                         (long)(a.hits - b.hits)};
    const char* names[4] = {"launches", "pool launches", "puts", "hits"};
    for (int k = 0; k < 4; k++)
      if (got[k] != want[k]) bad("pool", me, names[k], got[k], want[k]);
    if (a.used != (me == 0 ? kPairs : 0)) bad("pool", me, "slots in use", (long)a.used, me == 0 ? kPairs : 0);
    const std::vector<int> out = r.get();
    for (int i = 0; i < kPairs * 4; i++) {
      const int k = i / 4, o = i % 4;
      const int wantv = (k % 2 != me && (o == 1 || o == 2)) ? i + 1000 * other + 7 * it : -1;
      if (out[(size_t)i] != wantv) {
        bad("pool", me, "recvbuf[i]", out[(size_t)i], wantv);
        break;
      }
    }
    idle("pool", me, req);
  }
}

static void run_world(int P, const std::function<void(mpi::Intracomm&)>& fn) {
  std::vector<mpi::Intracomm> world = mpi::smp_world(P, std::vector<int>((size_t)P, 0));
  std::vector<std::thread> th;
  for (int r = 0; r < P; r++)
    th.emplace_back([&, r] {
      try {
        (void)hipSetDevice(0);
        world[(size_t)r].SetP2PTimeout(20);
        fn(world[(size_t)r]);
      } catch (const std::exception& e) {
        printf("rank %d: %s\n", r, e.what());
        g_bad++;
      }
    });
  for (auto& t : th) t.join();
}

int main() {
  run_world(2, reuse_test);
  printf("reuse TEST COMPLETE (P = 2)\n");
  run_world(4, halo_test);
  printf("halo TEST COMPLETE (P = 4)\n");
  run_world(2, [](mpi::Intracomm& c) { pool_test(c, 30, 2, 1); });
  printf("pool TEST COMPLETE (P = 2, 30 pairs)\n");
  run_world(2, [](mpi::Intracomm& c) { pool_test(c, 513, 22, 2); });
  printf("pool TEST COMPLETE (P = 2, 513 pairs)\n");
  if (g_bad.load()) {
    printf("%d FAILURES\n", g_bad.load());
    return 1;
  }
  printf("ALL PREQ TESTS PASSED\n");
  return 0;
}
