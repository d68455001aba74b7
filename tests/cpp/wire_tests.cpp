// wire_tests.cpp — MPI.PACKED messages, Probe and Iprobe written against the C++ host mirror (include/mpjx.hpp),
// run in multicore mode on GPU 0 with device arrays and one thread per rank (P = 2):
//   sections  Pack INT x 3 and a DOUBLE Vector column into one image, Send it PACKED twice; Recv PACKED and Unpack
//             both sections; a typed Recv(INT) of the same image gets section one only, its count from the header
//   probe     Iprobe sees nothing before the send; Probe(ANY_SOURCE, ANY_TAG) -> wire_bytes -> allocate ->
//             Recv(PACKED) -> Unpack; two probes give the same answer and the receive takes the message
// Left to tests/test_gpu_wire.py, which runs them from Python rank threads: every arm of k_wire in both
// directions, short messages, the errors, the launch counts and persistent requests.
//   build: make -C mpjexpress_amd tests     run: tests/cpp/wire_tests
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
  ~Dev() {
    (void)hipDeviceSynchronize();  // an eager send returns before its pack has run
    (void)hipFree(d);
  }
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
#define WANT(test, what, got, want)                                        \
  do {                                                                     \
    if ((long)(got) != (long)(want)) bad(test, me, what, (long)(got), (long)(want)); \
  } while (0)

static void sections_test(mpi::Intracomm& c) {
  const int me = c.Rank();
  mpi::Datatype col = mpi::Datatype::Vector(5, 1, 4, MPI::DOUBLE);  // a column of a 5 x 4 matrix
  std::vector<double> mat(20);
  for (int i = 0; i < 20; i++) mat[(size_t)i] = i + 0.5;
  if (me == 0) {
    Dev<int> ints({7, -8, 9});
    Dev<double> m(mat);
    Dev<unsigned char> img(std::vector<unsigned char>(128, 0));
    int64_t pos = c.Pack(ints.d, 0, 3, MPI::INT, img.d, 128, 0);
    WANT("sections", "position after INT x 3", pos, 20);
    pos = c.Pack(m.d, 2, 1, col, img.d, 128, pos);
    WANT("sections", "position after the column", pos, 72);
    c.Send(img.d, 0, (int)pos, MPI::PACKED, 1, 5);
    c.Send(img.d, 0, (int)pos, MPI::PACKED, 1, 6);
  } else {
    Dev<unsigned char> img(std::vector<unsigned char>(128, 0xA5));
    const mpi::Status st = c.Recv(img.d, 0, 100, MPI::PACKED, 0, 5);
    WANT("sections", "Get_count(PACKED)", st.Get_count(MPI::PACKED), 72);
    WANT("sections", "source", st.source, 0);
    const std::vector<unsigned char> h = img.get();
    WANT("sections", "type code of section 1", h[0], 4);
    WANT("sections", "count of section 1", h[7], 3);
    WANT("sections", "type code of section 2", h[24], 7);
    WANT("sections", "count of section 2", h[31], 5);
    WANT("sections", "byte past the message", h[72], 0xA5);
    Dev<int> gi(std::vector<int>(3, -1));
    Dev<double> gm(std::vector<double>(20, -1.0));
    int64_t pos = c.Unpack(img.d, 72, 0, gi.d, 0, 3, MPI::INT);
    pos = c.Unpack(img.d, 72, pos, gm.d, 1, 1, col);
    WANT("sections", "position after both", pos, 72);
    const std::vector<int> i3 = gi.get();
    WANT("sections", "ints[0]", i3[0], 7);
    WANT("sections", "ints[1]", i3[1], -8);
    WANT("sections", "ints[2]", i3[2], 9);
    const std::vector<double> g = gm.get();
    for (int i = 0; i < 20; i++) {
      const double want = i % 4 == 1 ? mat[(size_t)(i + 1)] : -1.0;
      if (g[(size_t)i] != want) bad("sections", me, "column element", (long)(g[(size_t)i] * 2), (long)(want * 2));
    }
    Dev<int> g8(std::vector<int>(8, -1));
    const mpi::Status s2 = c.Recv(g8.d, 0, 8, MPI::INT, 0, 6);  // the first section only
    WANT("sections", "Get_count(INT) of the typed receive", s2.Get_count(MPI::INT), 3);
    const std::vector<int> i8 = g8.get();
    const int want8[8] = {7, -8, 9, -1, -1, -1, -1, -1};
    for (int i = 0; i < 8; i++) WANT("sections", "typed receive element", i8[(size_t)i], want8[i]);
  }
  c.Barrier();
}

static void probe_test(mpi::Intracomm& c) {
  const int me = c.Rank();
  mpi::Datatype vec = mpi::Datatype::Vector(4, 2, 5, MPI::DOUBLE);
  std::vector<double> mat(20);
  for (int i = 0; i < 20; i++) mat[(size_t)i] = i * 1.5;
  Dev<double> src(mat);
  if (me == 1) WANT("probe", "Iprobe before the send", c.Iprobe(MPI::ANY_SOURCE, MPI::ANY_TAG), false);
  c.Barrier();
  if (me == 0) c.Send(src.d, 0, 1, vec, 1, 7);  // eager: it returns with the message unmatched
  c.Barrier();
  if (me == 1) {
    const mpi::Status a = c.Probe(MPI::ANY_SOURCE, MPI::ANY_TAG), b = c.Probe(0, 7);
    mpi::Status i;
    WANT("probe", "Iprobe after the send", c.Iprobe(0, MPI::ANY_TAG, &i), true);
    for (const mpi::Status* st : {&a, &b, (const mpi::Status*)&i}) {
      WANT("probe", "source", st->source, 0);
      WANT("probe", "tag", st->tag, 7);
      WANT("probe", "Get_count(DOUBLE)", st->Get_count(MPI::DOUBLE), 8);
      WANT("probe", "wire_bytes", st->wire_bytes(), 72);
    }
    Dev<unsigned char> img(std::vector<unsigned char>((size_t)a.wire_bytes(), 0));
    const mpi::Status st = c.Recv(img.d, 0, (int)a.wire_bytes(), MPI::PACKED, a.source, a.tag);
    WANT("probe", "Get_count(PACKED)", st.Get_count(MPI::PACKED), 72);
    Dev<double> out(std::vector<double>(20, -1.0));
    WANT("probe", "Unpack position", c.Unpack(img.d, 72, 0, out.d, 0, 1, vec), 72);
    const std::vector<double> g = out.get();
    for (int k = 0; k < 20; k++) {
      const double want = k % 5 < 2 ? mat[(size_t)k] : -1.0;
      if (g[(size_t)k] != want) bad("probe", me, "unpacked element", (long)(g[(size_t)k] * 2), (long)(want * 2));
    }
    WANT("probe", "Iprobe after the receive", c.Iprobe(MPI::ANY_SOURCE, MPI::ANY_TAG), false);
  }
  c.Barrier();
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
  run_world(2, sections_test);
  printf("sections TEST COMPLETE (P = 2)\n");
  run_world(2, probe_test);
  printf("probe TEST COMPLETE (P = 2)\n");
  if (g_bad.load()) {
    printf("%d FAILURES\n", g_bad.load());
    return 1;
  }
  printf("ALL WIRE TESTS PASSED\n");
  return 0;
}
