// strided_tests.cpp — the strided block moves through the C++ host mirror (include/mpjx.hpp: Datatype::Vector,
// Datatype::Contiguous) on GPU 0 with device arrays.
//   build: make -C mpjexpress_amd tests     run: tests/cpp/strided_tests [P ...]   (default P = 3)
//   - P = 1: packed lengths of one granule less than, exactly, and one granule more than one tile and two
//     tiles of k_strided (the tile comes from the planner's header), every other int of the source
//   - P = 1: one call past the streaming threshold (the non-temporal form), 4 KiB blocks at stride 8 KiB
//   - multicore at each P: Alltoallv with a Vector send type (ragged items) and Gatherv with a Vector
//     receive type (every rank's row lands as a column of the root's matrix); at P = 2 also one Alltoall past
//     the streaming threshold: four segments in one table of the non-temporal form
// Every receive array starts as a sentinel and is compared whole: a write into a gap fails.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>

#include "../../mpjexpress_amd/csrc/mpjx_strided_plan.hpp"
#include "mpjx.hpp"

using mpi::MPI;

static std::atomic<int> g_bad{0};
constexpr int SENT = -0x5a5a5a5b;

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
static void expect(const char* test, int rank, long tag, const std::vector<T>& got, const std::vector<T>& want) {
  for (size_t i = 0; i < want.size(); i++)
    if (got[i] != want[i]) {
      printf("%s (%ld) rank %d: received %lld at [%zu], should be %lld\n", test, tag, rank, (long long)got[i], i,
             (long long)want[i]);
      g_bad++;
      return;
    }
}

static void tile_edges(mpi::Intracomm& c) {
  const int tile = (int)mpjx::kStridedTile;  // granules of 4 B here: the blocks are single ints
  for (int n : {tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile, 2 * tile + 1}) {
    mpi::Datatype every_other = mpi::Datatype::Vector(n, 1, 2, MPI::INT);
    std::vector<int> out(2 * n + 3), want(n + 5, SENT);
    for (size_t i = 0; i < out.size(); i++) out[i] = (int)(i * 7 + 1);
    for (int i = 0; i < n; i++) want[2 + i] = out[1 + 2 * i];
    Dev<int> dout(out), din(std::vector<int>(n + 5, SENT));
    c.Alltoallv(dout.d, 1, {1}, {0}, every_other, din.d, 0, {n}, {2}, MPI::INT);
    expect("tile edge, gather", 0, n, din.get(), want);
    // and back into every other int of a sentinel array
    std::vector<int> back(2 * n + 3, SENT);
    for (int i = 0; i < n; i++) back[1 + 2 * i] = out[1 + 2 * i];
    Dev<int> dback(std::vector<int>(2 * n + 3, SENT));
    c.Alltoallv(din.d, 2, {n}, {0}, MPI::INT, dback.d, 0, {1}, {1}, every_other);
    expect("tile edge, scatter", 0, n, dback.get(), back);
    every_other.Free();
  }
}

static void streaming_form(mpi::Intracomm& c) {
  // 64 MiB + 3 blocks of packed doubles in 4 KiB blocks at stride 8 KiB: at least mpjx::kStridedStreamBytes
  const int bl = 512, nblocks = (int)(mpjx::kStridedStreamBytes / (bl * 8)) + 3;
  mpi::Datatype panel = mpi::Datatype::Vector(nblocks, bl, 2 * bl, MPI::DOUBLE);
  std::vector<long long> out((size_t)panel.Extent() + 2), want((size_t)nblocks * bl + 4, SENT);
  for (size_t i = 0; i < out.size(); i++) out[i] = (long long)(i * 2654435761u) ^ (long long)i << 32;
  for (int b = 0; b < nblocks; b++)
    for (int w = 0; w < bl; w++) want[2 + (size_t)b * bl + w] = out[2 + (size_t)b * 2 * bl + w];
  Dev<long long> dout(out), din(std::vector<long long>(want.size(), SENT));
  c.Alltoallv((const double*)dout.d, 2, {1}, {0}, panel, (double*)din.d, 0, {nblocks * bl}, {2}, MPI::DOUBLE);
  expect("streaming form", 0, nblocks, din.get(), want);
  panel.Free();
}

static int ragged(int i, int j) { return (7 * i + 3 * j) % 5 == 0 ? 0 : 1 + (13 * i + 7 * j) % 4; }

static void alltoallv_vector(mpi::Intracomm& c) {
  const int P = c.Size(), me = c.Rank();
  mpi::Datatype v = mpi::Datatype::Vector(3, 2, 5, MPI::INT);  // 6 ints of data, extent 12
  std::vector<int> sc(P), sd(P), rc(P), rd(P);
  int spos = 1, rpos = 2;
  for (int j = 0; j < P; j++) {
    sc[j] = ragged(me, j);
    sd[j] = spos;
    spos += sc[j] * v.Extent() + 1 + j % 3;
    rc[j] = ragged(j, me) * v.Size();
    rd[j] = rpos;
    rpos += rc[j] + 2;
  }
  std::vector<int> out(spos + 4), want(rpos + 4, SENT);
  for (size_t i = 0; i < out.size(); i++) out[i] = me * 100000 + (int)i;
  for (int i = 0; i < P; i++) {  // what rank i sends to me: its displacement table is built the same way
    int pos = 1;
    for (int j = 0; j < me; j++) pos += ragged(i, j) * v.Extent() + 1 + j % 3;
    int at = rd[i];
    for (int k = 0; k < ragged(i, me); k++)
      for (int b = 0; b < 3; b++)
        for (int w = 0; w < 2; w++) want[at++] = i * 100000 + pos + k * v.Extent() + b * 5 + w;
  }
  Dev<int> dout(out), din(std::vector<int>(want.size(), SENT));
  c.Alltoallv(dout.d, 0, sc, sd, v, din.d, 0, rc, rd, MPI::INT);
  expect("Alltoallv(Vector)", me, P, din.get(), want);
  expect("Alltoallv(Vector) sendbuf", me, P, dout.get(), out);
  v.Free();
}

static void gatherv_columns(mpi::Intracomm& c) {
  const int P = c.Size(), me = c.Rank(), rows = 5, root = P - 1;
  mpi::Datatype col = mpi::Datatype::Vector(rows, 1, P, MPI::DOUBLE);  // a column of the root's rows x P matrix
  std::vector<double> out(rows);
  for (int k = 0; k < rows; k++) out[k] = me * 10 + k + 0.5;
  std::vector<int> rc(P, 1), rd(P);
  for (int j = 0; j < P; j++) rd[j] = j;  // base elements: column j starts one double after column j - 1
  std::vector<double> want((size_t)rows * P + 2, -1.0);
  if (me == root)
    for (int j = 0; j < P; j++)
      for (int k = 0; k < rows; k++) want[1 + (size_t)k * P + j] = j * 10 + k + 0.5;
  Dev<double> dout(out), din(std::vector<double>(want.size(), -1.0));
  c.Gatherv(dout.d, 0, rows, MPI::DOUBLE, din.d, 1, rc, rd, col, root);
  expect("Gatherv(columns)", me, P, din.get(), want);
  col.Free();
}

static void alltoall_streaming(mpi::Intracomm& c) {
  // P = 2: four segments of 16 MiB + 4 KiB packed each, 4 KiB blocks at stride 8 KiB into plain doubles
  const int P = c.Size(), me = c.Rank(), bl = 512, nblocks = (int)(mpjx::kStridedStreamBytes / 4 / (bl * 8)) + 1;
  mpi::Datatype panel = mpi::Datatype::Vector(nblocks, bl, 2 * bl, MPI::DOUBLE);
  const size_t per = (size_t)nblocks * bl;
  std::vector<long long> out((size_t)P * panel.Extent() + 1), want(P * per + 2, SENT);
  for (size_t i = 0; i < out.size(); i++) out[i] = (long long)(i * 2654435761u + (size_t)me);
  for (int i = 0; i < P; i++)  // rank i's block `me` starts me extents into its buffer (offset 1)
    for (int b = 0; b < nblocks; b++)
      for (int w = 0; w < bl; w++)
        want[1 + i * per + (size_t)b * bl + w] =
            (long long)((1 + (size_t)me * panel.Extent() + (size_t)b * 2 * bl + w) * 2654435761u + (size_t)i);
  Dev<long long> dout(out), din(std::vector<long long>(want.size(), SENT));
  c.Alltoall((const double*)dout.d, 1, 1, panel, (double*)din.d, 1, (int)per, MPI::DOUBLE);
  expect("Alltoall, streaming form", me, nblocks, din.get(), want);
  panel.Free();
}

int main(int argc, char** argv) {
  std::vector<int> Ps;
  for (int a = 1; a < argc; a++) Ps.push_back(atoi(argv[a]));
  if (Ps.empty()) Ps.push_back(3);
  try {
    {
      std::vector<mpi::Intracomm> w = mpi::smp_world(1, {0});
      tile_edges(w[0]);
      streaming_form(w[0]);
    }
    for (int P : Ps) {
      std::vector<mpi::Intracomm> w = mpi::smp_world(P, std::vector<int>(P, 0));
      std::vector<std::thread> th;
      for (int r = 0; r < P; r++)
        th.emplace_back([&w, r] {
          try {
            (void)hipSetDevice(0);
            alltoallv_vector(w[r]);
            gatherv_columns(w[r]);
            if (w[r].Size() == 2) alltoall_streaming(w[r]);
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
    printf("%d STRIDED TESTS FAILED\n", g_bad.load());
    return 1;
  }
  printf("ALL STRIDED TESTS PASSED\n");
  return 0;
}
