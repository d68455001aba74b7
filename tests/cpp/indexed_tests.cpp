// indexed_tests.cpp — the irregular datatypes through the C++ host mirror (include/mpjx.hpp: Datatype::Indexed,
// Datatype::Hindexed, Datatype::Hvector) on GPU 0 with device arrays.
//   build: make -C mpjexpress_amd tests     run: tests/cpp/indexed_tests [P ...]   (default P = 3)
//   - the mirror's Size / Extent / Lb / Ub, and its exceptions
//   - P = 1: the upper triangle of an 8 x 8 matrix (test/mpi/dtyp/Indexed.java) packed into 36 doubles and
//     unpacked into another matrix; an Hvector of a Vector (hvec.java) against the same walk on the host
//   - multicore at each P: Alltoallv with an Indexed send type (ragged items) into plain ints
// Every receive array starts as a sentinel and is compared whole: a write into a gap fails.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "mpjx.hpp"

using mpi::MPI;

static std::atomic<int> g_bad{0};
constexpr int SENT = -0x5a5a5a5b;
#define EXPECT(cond)                                         \
  do {                                                       \
    if (!(cond)) {                                           \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      g_bad++;                                               \
    }                                                        \
  } while (0)

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

template <class T>
static void expect(const char* test, int rank, const std::vector<T>& got, const std::vector<T>& want) {
  for (size_t i = 0; i < want.size(); i++)
    if (got[i] != want[i]) {
      printf("%s rank %d: received %g at [%zu], should be %g\n", test, rank, (double)got[i], i, (double)want[i]);
      g_bad++;
      return;
    }
}

static void mirror_types() {
  mpi::Datatype a = mpi::Datatype::Indexed({2, 1}, {9, 4}, MPI::INT);
  EXPECT(a.Size() == 3 && a.Extent() == 7 && a.Lb() == 4 && a.Ub() == 11 && a.Base() == MPJX_INT);
  mpi::Datatype h = mpi::Datatype::Hindexed({2, 1}, {18, 8}, MPI::DOUBLE2);
  EXPECT(h.Size() == 6 && h.Extent() == 14 && h.Lb() == 8 && h.Ub() == 22);
  mpi::Datatype v = mpi::Datatype::Vector(2, 3, 4, MPI::INT), hv = mpi::Datatype::Hvector(3, 1, 9, v);
  EXPECT(hv.Size() == 18 && hv.Extent() == 25 && hv.Lb() == 0 && v.Lb() == 0 && v.Ub() == 7 && MPI::INT.Ub() == 1);
  int threw = 0;
  try {
    mpi::Datatype::Indexed({1}, {-1}, MPI::INT);
  } catch (const mpi::MPIException&) { threw++; }
  try {
    mpi::Datatype::Indexed({1, 2}, {0}, MPI::INT);
  } catch (const mpi::MPIException&) { threw++; }
  try {
    mpi::Datatype::Hvector(2, 1, 0, MPI::INT);
  } catch (const mpi::MPIException&) { threw++; }
  EXPECT(threw == 3);
  a.Free(), h.Free(), hv.Free(), v.Free();
}

static void triangle(mpi::Intracomm& c) {
  std::vector<int> bl, ds;
  for (int i = 0; i < 8; i++) bl.push_back(8 - i), ds.push_back(9 * i);
  mpi::Datatype tri = mpi::Datatype::Indexed(bl, ds, MPI::DOUBLE);
  std::vector<double> m(64), packed(38, SENT), back(66, SENT), want_p(38, SENT), want_b(66, SENT);
  for (int i = 0; i < 64; i++) m[i] = i + 0.5;
  int k = 0;
  for (int i = 0; i < 8; i++)
    for (int j = i; j < 8; j++) want_p[1 + k++] = m[8 * i + j], want_b[1 + 8 * i + j] = m[8 * i + j];
  Dev<double> dm(m), dp(packed), db(back);
  c.Alltoall(dm.d, 0, 1, tri, dp.d, 1, 36, MPI::DOUBLE);
  c.Alltoall(dp.d, 1, 36, MPI::DOUBLE, db.d, 1, 1, tri);
  expect("triangle pack", 0, dp.get(), want_p);
  expect("triangle unpack", 0, db.get(), want_b);
  // hvec.java's shape with two items: Hvector(3, 1, 9, Vector(2, 3, 4, INT)), extent 25
  mpi::Datatype v = mpi::Datatype::Vector(2, 3, 4, MPI::INT), hv = mpi::Datatype::Hvector(3, 1, 9, v);
  std::vector<int> src(60), got(40, SENT), want(40, SENT);
  for (int i = 0; i < 60; i++) src[i] = 3 * i + 1;
  k = 2;
  for (int item = 0; item < 2; item++)
    for (int j = 0; j < 3; j++)
      for (int b = 0; b < 2; b++)
        for (int w = 0; w < 3; w++) want[k++] = src[1 + 25 * item + 9 * j + 4 * b + w];
  Dev<int> ds_(src), dg(got);
  c.Alltoall(ds_.d, 1, 2, hv, dg.d, 2, 36, MPI::INT);
  expect("hvector of vector", 0, dg.get(), want);
  tri.Free(), hv.Free(), v.Free();
}

static void world(int P) {
  std::vector<mpi::Intracomm> comms = mpi::smp_world(P, std::vector<int>(P, 0));
  std::vector<std::thread> th;
  for (int r = 0; r < P; r++)
    th.emplace_back([&, r] {
      try {
        (void)hipSetDevice(0);
        mpi::Intracomm& c = comms[r];
        mpi::Datatype t = mpi::Datatype::Indexed({3, 1, 2}, {8, 0, 4}, MPI::INT);  // extent 11, 6 ints
        auto items = [](int i, int j) { return (i + 2 * j) % 3; };  // rank i sends rank j this many
        std::vector<int> sc(P), sd(P), rc(P), rd(P);
        int at = 1, rat = 2;
        for (int j = 0; j < P; j++) sc[j] = items(r, j), sd[j] = at, at += 11 * sc[j] + 2;
        for (int i = 0; i < P; i++) rc[i] = 6 * items(i, r), rd[i] = rat, rat += rc[i] + 1;
        auto value = [](int rank, int i) { return 1000 * rank + i; };
        std::vector<int> src(at + 2), want(rat + 2, SENT);
        for (size_t i = 0; i < src.size(); i++) src[i] = value(r, (int)i);
        for (int i = 0; i < P; i++) {  // what rank i packs for this rank, from its own displacement table
          int iat = 1;
          for (int j = 0; j < r; j++) iat += 11 * items(i, j) + 2;
          int k = rd[i];
          const int off[3] = {8, 0, 4}, len[3] = {3, 1, 2};
          for (int it = 0; it < items(i, r); it++)
            for (int b = 0; b < 3; b++)
              for (int w = 0; w < len[b]; w++) want[k++] = value(i, iat + 11 * it + off[b] + w);
        }
        Dev<int> ds(src), dr(std::vector<int>(want.size(), SENT));
        c.Alltoallv(ds.d, 0, sc, sd, t, dr.d, 0, rc, rd, MPI::INT);
        expect("alltoallv indexed", r, dr.get(), want);
        t.Free();
      } catch (const std::exception& e) {
        printf("rank %d: %s\n", r, e.what());
        g_bad++;
      }
    });
  for (std::thread& t : th) t.join();
}

int main(int argc, char** argv) {
  std::vector<int> Ps;
  for (int i = 1; i < argc; i++) Ps.push_back(atoi(argv[i]));
  if (Ps.empty()) Ps.push_back(3);
  (void)hipSetDevice(0);
  mirror_types();
  {
    std::vector<mpi::Intracomm> one = mpi::smp_world(1, {0});
    triangle(one[0]);
  }
  for (int P : Ps) {
    world(P);
    printf("P = %d: TEST COMPLETE\n", P);
  }
  if (g_bad) {
    printf("%d FAILURES\n", g_bad.load());
    return 1;
  }
  printf("ALL INDEXED TESTS PASSED\n");
  return 0;
}
