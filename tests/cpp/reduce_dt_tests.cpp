// reduce_dt_tests.cpp — the reductions on a derived datatype through the C++ host mirror (include/mpjx.hpp) on
// GPU 0 with device arrays, multicore rank threads on one device.
//   build: make -C mpjexpress_amd tests     run: tests/cpp/reduce_dt_tests [P ...]   (default P = 4)
//   - Allreduce(SUM), Scan(SUM) and Reduce_scatter(MAX, ragged recvcounts with a 0) on Vector(6, 2, 5, INT):
//     integer data, so the expectation is computed here whatever the combine order
//   - every call must take the layout-direct form (mpjx_comm_last_dt_form)
//   - a derived type on host vectors throws
// Every receive array starts as a sentinel and is compared whole: a write into a gap fails.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "mpjx.hpp"

using mpi::MPI;

static std::atomic<int> g_bad{0};
constexpr int SENT = -0x5a5a5a5b;
constexpr int NB = 6, BL = 2, ST = 5;  // Vector(6, 2, 5): 12 ints of data, extent 27

struct Dev {
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
      printf("%s rank %d: received %d at [%zu], should be %d\n", test, rank, got[i], i, want[i]);
      g_bad++;
      return;
    }
}

static void direct_form(mpi::Intracomm& c, const char* test) {
  int form = -1;
  mpi::check(mpjx_comm_last_dt_form(c.handle(), &form), "mpjx_comm_last_dt_form");
  if (form != MPJX_DT_FORM_DIRECT) {
    printf("%s rank %d: took form %d, not the layout-direct kernel\n", test, c.Rank(), form);
    g_bad++;
  }
}

static int value(int rank, int i) { return (rank + 1) * 1000 + 3 * i - 40 * (i % 7); }
// index of packed element e of item k, from the buffer position
static int at(int k, int e, int extent) { return k * extent + (e / BL) * ST + e % BL; }

static void reductions(mpi::Intracomm& c) {
  const int P = c.Size(), me = c.Rank(), count = 3, soff = 1, roff = 2;
  mpi::Datatype v = mpi::Datatype::Vector(NB, BL, ST, MPI::INT);
  const int ext = v.Extent(), per = v.Size();
  std::vector<int> out((size_t)soff + count * ext + 3);
  for (size_t i = 0; i < out.size(); i++) out[i] = value(me, (int)i);
  {  // Allreduce(SUM)
    std::vector<int> want((size_t)roff + count * ext + 3, SENT);
    for (int k = 0; k < count; k++)
      for (int e = 0; e < per; e++) {
        int s = 0;
        for (int r = 0; r < P; r++) s += value(r, soff + at(k, e, ext));
        want[roff + at(k, e, ext)] = s;
      }
    Dev dout(out), din(std::vector<int>(want.size(), SENT));
    c.Allreduce(dout.d, soff, din.d, roff, count, v, MPI::SUM);
    direct_form(c, "Allreduce(Vector)");
    expect("Allreduce(Vector)", me, din.get(), want);
    expect("Allreduce(Vector) sendbuf", me, dout.get(), out);
  }
  {  // Scan(SUM): ranks 0..me
    std::vector<int> want((size_t)roff + count * ext + 3, SENT);
    for (int k = 0; k < count; k++)
      for (int e = 0; e < per; e++) {
        int s = 0;
        for (int r = 0; r <= me; r++) s += value(r, soff + at(k, e, ext));
        want[roff + at(k, e, ext)] = s;
      }
    Dev dout(out), din(std::vector<int>(want.size(), SENT));
    c.Scan(dout.d, soff, din.d, roff, count, v, MPI::SUM);
    direct_form(c, "Scan(Vector)");
    expect("Scan(Vector)", me, din.get(), want);
  }
  {  // Reduce_scatter(MAX): rank r receives recvcounts[r] items from its receive buffer's own origin
    std::vector<int> rc(P);
    int total = 0, mine0 = 0;
    for (int r = 0; r < P; r++) {
      rc[r] = (r * 2 + 1) % 3;  // 1, 0, 2, 1, ...
      if (r < me) mine0 += rc[r];
      total += rc[r];
    }
    std::vector<int> big((size_t)soff + total * ext + 3);
    for (size_t i = 0; i < big.size(); i++) big[i] = value(me, (int)i) * ((int)i % 2 ? 1 : -1);
    std::vector<int> want((size_t)roff + rc[me] * ext + 3, SENT);
    for (int k = 0; k < rc[me]; k++)
      for (int e = 0; e < per; e++) {
        const int i = soff + at(mine0 + k, e, ext);
        int m = value(0, i) * (i % 2 ? 1 : -1);
        for (int r = 1; r < P; r++) m = std::max(m, value(r, i) * (i % 2 ? 1 : -1));
        want[roff + at(k, e, ext)] = m;
      }
    Dev dout(big), din(std::vector<int>(want.size(), SENT));
    c.Reduce_scatter(dout.d, soff, din.d, roff, rc, v, MPI::MAX);
    direct_form(c, "Reduce_scatter(Vector)");
    expect("Reduce_scatter(Vector)", me, din.get(), want);
  }
  v.Free();
}

static void host_vectors_throw() {
  std::vector<mpi::Intracomm> w = mpi::smp_world(1, {0});
  mpi::Datatype v = mpi::Datatype::Vector(NB, BL, ST, MPI::INT);
  std::vector<int> a(64, 1), b(64, 0);
  bool threw = false;
  try {
    w[0].Allreduce(a, 0, b, 0, 1, v, MPI::SUM);
  } catch (const mpi::MPIException&) {
    threw = true;
  }
  if (!threw || b[0] != 0) {
    printf("Allreduce(Vector) on host vectors did not throw\n");
    g_bad++;
  }
  v.Free();
}

int main(int argc, char** argv) {
  std::vector<int> Ps;
  for (int a = 1; a < argc; a++) Ps.push_back(atoi(argv[a]));
  if (Ps.empty()) Ps.push_back(4);
  try {
    host_vectors_throw();
    for (int P : Ps) {
      std::vector<mpi::Intracomm> w = mpi::smp_world(P, std::vector<int>(P, 0));
      std::vector<std::thread> th;
      for (int r = 0; r < P; r++)
        th.emplace_back([&w, r] {
          try {
            (void)hipSetDevice(0);
            reductions(w[r]);
          } catch (const std::exception& e) {
            printf("rank %d: %s\n", r, e.what());
            g_bad++;
          }
        });
      for (std::thread& t : th) t.join();
      printf("P = %d: TEST COMPLETE\n", P);
    }
  } catch (const std::exception& e) {
    printf("%s\n", e.what());
    g_bad++;
  }
  if (g_bad) {
    printf("%d REDUCE_DT TESTS FAILED\n", g_bad.load());
    return 1;
  }
  printf("ALL REDUCE_DT TESTS PASSED\n");
  return 0;
}
