// pack_tests.cpp — Pack / Unpack / Pack_size through the C++ host mirror (include/mpjx.hpp) on GPU 0.
//   build: make -C mpjexpress_amd tests     run: tests/cpp/pack_tests
//   - Pack_size's known values
//   - two sections in one device image: BYTE x 3 at 0, Vector(3, 2, 5, INT) x 2 from position 11; the image is
//     compared whole against bytes written here by hand, both are unpacked into sentinel arrays
//   - an Hindexed of DOUBLE (lb = 1) round trip
//   - Unpack of a section of another type throws and leaves the array untouched
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mpjx.hpp"

using mpi::MPI;

static int g_bad = 0;
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
static void put_be(std::vector<unsigned char>& img, size_t at, T v) {  // one base word, big-endian
  unsigned char b[sizeof(T)];
  memcpy(b, &v, sizeof(T));
  for (size_t i = 0; i < sizeof(T); i++) img[at + i] = b[sizeof(T) - 1 - i];
}
static void put_header(std::vector<unsigned char>& img, size_t h, int base, int words) {
  img[h] = (unsigned char)(base - 1);
  img[h + 1] = img[h + 2] = img[h + 3] = 0;
  put_be<int>(img, h + 4, words);
}

static void two_sections(mpi::Intracomm& c) {
  EXPECT(c.Pack_size(1, MPI::BYTE) == 10 && c.Pack_size(3, MPI::BYTE) == 14 && c.Pack_size(1, MPI::SHORT) == 12);
  EXPECT(c.Pack_size(1, MPI::INT) == 16 && c.Pack_size(1, MPI::DOUBLE) == 16);
  mpi::Datatype v = mpi::Datatype::Vector(3, 2, 5, MPI::INT);  // extent 12, 6 ints
  EXPECT(c.Pack_size(2, v) == 56);
  const std::vector<signed char> by = {-3, 7, 100};
  std::vector<int> src(30);
  for (int i = 0; i < 30; i++) src[(size_t)i] = 0x01020304 * (i + 1) - 77;
  std::vector<unsigned char> img(80, 0xA5), want(80, 0xA5);
  put_header(want, 0, MPJX_BYTE, 3);
  for (int i = 0; i < 3; i++) want[8 + (size_t)i] = (unsigned char)by[(size_t)i];
  put_header(want, 16, MPJX_INT, 12);
  size_t at = 24;
  for (int k = 0; k < 2; k++)
    for (int b = 0; b < 3; b++)
      for (int w = 0; w < 2; w++, at += 4) put_be<int>(want, at, src[(size_t)(1 + 12 * k + 5 * b + w)]);
  Dev<signed char> dby(by);
  Dev<int> dsrc(src);
  Dev<unsigned char> dimg(img);
  int64_t pos = c.Pack(dby.d, 0, 3, MPI::BYTE, dimg.d, 80, 0);
  EXPECT(pos == 11);
  pos = c.Pack(dsrc.d, 1, 2, v, dimg.d, 80, pos);
  EXPECT(pos == 72);
  EXPECT(dimg.get() == want);  // bytes 11..15 and 72..79 keep the fill
  Dev<signed char> oby(std::vector<signed char>(5, 0x5A));
  Dev<int> osrc(std::vector<int>(30, 0x5A5A5A5A));
  pos = c.Unpack(dimg.d, 80, 0, oby.d, 1, 3, MPI::BYTE);
  EXPECT(pos == 11);
  pos = c.Unpack(dimg.d, 80, pos, osrc.d, 1, 2, v);
  EXPECT(pos == 72);
  EXPECT(oby.get() == (std::vector<signed char>{0x5A, -3, 7, 100, 0x5A}));
  std::vector<int> back(30, 0x5A5A5A5A);
  for (int k = 0; k < 2; k++)
    for (int b = 0; b < 3; b++)
      for (int w = 0; w < 2; w++) back[(size_t)(1 + 12 * k + 5 * b + w)] = src[(size_t)(1 + 12 * k + 5 * b + w)];
  EXPECT(osrc.get() == back);
  // a section of another type: the kernel reports it, the mirror throws, the array keeps its contents
  Dev<int> keep(std::vector<int>(30, 0x5A5A5A5A));
  int threw = 0;
  try {
    c.Unpack(dimg.d, 80, 0, keep.d, 0, 3, MPI::INT);  // BYTE x 3 is there; INT x 3 would also pass its end
  } catch (const mpi::MPIException&) { threw++; }
  try {
    c.Unpack(dimg.d, 80, 11, keep.d, 0, 12, MPI::FLOAT);  // the count and the room fit: the type code differs
  } catch (const mpi::MPIException& e) { threw += strstr(e.what(), "status 1") != nullptr; }
  try {
    c.Unpack(dimg.d, 80, 11, keep.d, 0, 11, MPI::INT);  // one element short of the header's count
  } catch (const mpi::MPIException& e) { threw += strstr(e.what(), "status 2") != nullptr; }
  EXPECT(threw == 3);
  EXPECT(keep.get() == std::vector<int>(30, 0x5A5A5A5A));
  v.Free();
}

static void hindexed_round_trip(mpi::Intracomm& c) {
  mpi::Datatype t = mpi::Datatype::Hindexed({2, 2, 2}, {1, 11, 5}, MPI::DOUBLE);  // lb 1, extent 12, 6 doubles
  EXPECT(t.Lb() == 1 && t.Extent() == 12 && t.Size() == 6);
  std::vector<double> src(40);
  for (int i = 0; i < 40; i++) src[(size_t)i] = 1.0 / (i + 3);
  const int off[3] = {1, 11, 5};
  std::vector<unsigned char> img(8 + 8 + 18 * 8 + 8, 0xA5), want(img);
  put_header(want, 8, MPJX_DOUBLE, 18);
  size_t at = 16;
  std::vector<double> back(40, -1.0);
  for (int k = 0; k < 3; k++)
    for (int b = 0; b < 3; b++)
      for (int w = 0; w < 2; w++, at += 8) {
        const size_t i = (size_t)(2 + 12 * k + off[b] + w);
        put_be<double>(want, at, src[i]);
        back[i] = src[i];
      }
  Dev<double> ds(src), dout(std::vector<double>(40, -1.0));
  Dev<unsigned char> dimg(img);
  EXPECT(c.Pack(ds.d, 2, 3, t, dimg.d, (int64_t)img.size(), 3) == 16 + 18 * 8);
  EXPECT(dimg.get() == want);
  EXPECT(c.Unpack(dimg.d, (int64_t)img.size(), 3, dout.d, 2, 3, t) == 16 + 18 * 8);
  EXPECT(dout.get() == back);
  t.Free();
}

int main() {
  (void)hipSetDevice(0);
  try {
    std::vector<mpi::Intracomm> one = mpi::smp_world(1, {0});
    two_sections(one[0]);
    hindexed_round_trip(one[0]);
  } catch (const std::exception& e) {
    printf("exception: %s\n", e.what());
    g_bad++;
  }
  if (g_bad) {
    printf("%d FAILURES\n", g_bad);
    return 1;
  }
  printf("ALL PACK TESTS PASSED\n");
  return 0;
}
