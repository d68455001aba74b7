// p2p_tests.cpp — the reference's test/mpi/pt2pt/sendrecv.java and a 2 x 2 periodic halo exchange (4 Irecv + 4
// Isend + Waitall per rank: rows contiguous, columns Datatype::Vector) written against the C++ host mirror
// (include/mpjx.hpp), run in multicore mode on GPU 0 with device arrays and one thread per rank.
//   build: make -C mpjexpress_amd tests     run: tests/cpp/p2p_tests [P ...]   (default P = 4; the halo runs at 4)
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
    (void)hipMemcpy(d, h.data(), n * sizeof(T), hipMemcpyHostToDevice);
  }
  ~Dev() { (void)hipFree(d); }
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

static void sendrecv_step(mpi::Intracomm& c, int src, int dest) {
  const int me = c.Rank();
  std::vector<int> sendbuf(1000, 0), recvbuf(1000, 0);
  for (int i = 0; i < 100; i++) sendbuf[i] = me, recvbuf[i] = -1;
  Dev<int> s(sendbuf), r(recvbuf);
  const mpi::Status st = c.Sendrecv(s.d, 0, 100, MPI::INT, dest, me, r.d, 0, 100, MPI::INT, src, src);
  const std::vector<int> got = r.get();
  for (int i = 0; i < 1000; i++)
    if (got[i] != (i < 100 ? src : 0)) {
      bad("sendrecv", me, "recvbuf[i]", got[i], i < 100 ? src : 0);
      break;
    }
  if (s.get() != sendbuf) bad("sendrecv", me, "sendbuf changed", 1, 0);
  if (st.source != src) bad("sendrecv", me, "status.source", st.source, src);
  if (st.tag != src) bad("sendrecv", me, "status.tag", st.tag, src);
  if (st.Get_count(MPI::INT) != 100) bad("sendrecv", me, "Get_count", st.Get_count(MPI::INT), 100);
}

static void sendrecv_test(mpi::Intracomm& c) {  // sendrecv.java
  const int tasks = c.Size(), me = c.Rank();
  if (me < 2 && tasks >= 2) sendrecv_step(c, 1 - me, 1 - me);
  sendrecv_step(c, me == 0 ? tasks - 1 : me - 1, me == tasks - 1 ? 0 : me + 1);
  c.Barrier();
}

constexpr int N = 34;
static std::vector<double> tile_of(int rank) {
  std::vector<double> t((size_t)N * N);
  for (int i = 0; i < N * N; i++) t[(size_t)i] = rank * 10000.0 + i;
  return t;
}

static void halo_test(mpi::Intracomm& c) {
  const int me = c.Rank(), i = me / 2, j = me % 2;
  const int north = ((i + 1) % 2) * 2 + j, south = north, west = i * 2 + (j + 1) % 2, east = west;
  mpi::Datatype col = mpi::Datatype::Vector(N - 2, 1, N, MPI::DOUBLE);
  Dev<double> t(tile_of(me));
  std::vector<mpi::Request> req;
  req.push_back(c.Irecv(t.d, (N - 1) * N + 1, N - 2, MPI::DOUBLE, south, 0));
  req.push_back(c.Irecv(t.d, 1, N - 2, MPI::DOUBLE, north, 1));
  req.push_back(c.Irecv(t.d, N + N - 1, 1, col, east, 2));
  req.push_back(c.Irecv(t.d, N, 1, col, west, 3));
  req.push_back(c.Isend(t.d, N + 1, N - 2, MPI::DOUBLE, north, 0));
  req.push_back(c.Isend(t.d, (N - 2) * N + 1, N - 2, MPI::DOUBLE, south, 1));
  req.push_back(c.Isend(t.d, N + 1, 1, col, west, 2));
  req.push_back(c.Isend(t.d, N + N - 2, 1, col, east, 3));
  const std::vector<mpi::Status> st = mpi::Request::Waitall(req);
  for (int k = 0; k < 4; k++) {
    if (st[(size_t)k].tag != k) bad("halo", me, "status.tag", st[(size_t)k].tag, k);
    if (st[(size_t)k].Get_count(MPI::DOUBLE) != N - 2) bad("halo", me, "Get_count", st[(size_t)k].Get_count(MPI::DOUBLE), N - 2);
  }
  for (mpi::Request& r : req)
    if (!r.Is_null()) bad("halo", me, "request not null after Waitall", 1, 0);
  std::vector<double> want = tile_of(me);
  const std::vector<double> s = tile_of(south), n = tile_of(north), e = tile_of(east), w = tile_of(west);
  for (int k = 1; k < N - 1; k++) {
    want[(size_t)((N - 1) * N + k)] = s[(size_t)(N + k)];
    want[(size_t)k] = n[(size_t)((N - 2) * N + k)];
    want[(size_t)(k * N + N - 1)] = e[(size_t)(k * N + 1)];
    want[(size_t)(k * N)] = w[(size_t)(k * N + N - 2)];
  }
  const std::vector<double> got = t.get();
  for (int k = 0; k < N * N; k++)
    if (got[(size_t)k] != want[(size_t)k]) {
      bad("halo", me, "tile element", (long)got[(size_t)k], (long)want[(size_t)k]);
      break;
    }
  c.Barrier();
  col.Free();
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

int main(int argc, char** argv) {
  std::vector<int> Ps;
  for (int i = 1; i < argc; i++) Ps.push_back(atoi(argv[i]));
  if (Ps.empty()) Ps.push_back(4);
  for (int P : Ps) {
    run_world(P, sendrecv_test);
    printf("sendrecv TEST COMPLETE (P = %d)\n", P);
  }
  run_world(4, halo_test);
  printf("halo TEST COMPLETE (P = 4)\n");
  if (g_bad.load()) {
    printf("%d FAILURES\n", g_bad.load());
    return 1;
  }
  printf("ALL P2P TESTS PASSED\n");
  return 0;
}
