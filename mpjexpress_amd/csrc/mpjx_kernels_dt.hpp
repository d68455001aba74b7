// mpjx_kernels_dt.hpp — k_pway_dt: the P-way element-wise combine of k_pway (mpjx_kernels.hpp) over a derived
// datatype's layout, for the reductions that take one (mpjx_*_dt, planned by mpjx_reduce_dt_plan.hpp).
//
// Every operand and every output of a reduction has the SAME layout, so a lane computes the byte offset of
// its packed granule once (reduce_dt_offset: k_strided's FastDiv multiply-highs for a regular layout, the
// binary search of the type's device table for an irregular one; the kind is uniform per launch, a scalar
// branch), issues its P loads at in[p] + offset, evaluates the reference's combine ORDER with k_pway's
// eval_elem and functors, and stores at out[r] + offset: nrep copies for K_FOLD / K_MST (the multicore
// all-gather fused in), P outputs for K_SCAN. Bytes outside the layout's blocks are never touched.
//   W = 1            one element (a base element, or one (value, index) pair) per granule: any alignment
//   W = 16 / sizeof  a 16-B granule, where the host's rule gave it (reduce_dt_granule_log)
// The tile is the cache-resident form's: kThreads lanes x DtUnroll granules per lane, the default cache
// policy. Loads and stores go through global-address-space pointers, as in k_moves and k_strided.
#pragma once
#include "mpjx_kernels.hpp"
#include "mpjx_reduce_dt_plan.hpp"

namespace mpjx {

using v2u_dt = unsigned int __attribute__((ext_vector_type(2)));

// What one load or store moves: a granule of N bytes
template <int N>
struct DtGranule;
template <>
struct DtGranule<1> { using type = unsigned char; };
template <>
struct DtGranule<2> { using type = unsigned short; };
template <>
struct DtGranule<4> { using type = unsigned int; };
template <>
struct DtGranule<8> { using type = v2u_dt; };
template <>
struct DtGranule<16> { using type = v4u; };

constexpr uint32_t dt_log2(int n) { return n <= 1 ? 0 : 1 + dt_log2(n / 2); }

// Granules in flight per lane: k_pway's cache-resident unroll, one step shallower where P x W elements plus
// the offsets would not stay in registers (narrow types in the 16-B form at large P)
template <int P, int W>
struct DtUnroll {
  static constexpr int value = (W >= 8 && P >= 3) ? 1 : Unroll<P>::value;
};

template <class F, int P, int KIND, int W>
__global__ __launch_bounds__(kThreads) void k_pway_dt(PwayDtArgs a) {
  using T = typename F::T;
  static_assert(sizeof(typename Pack<T, W>::type) == W * sizeof(T), "W = 1, or a 16-B vector");
  constexpr int GB = W * (int)sizeof(T);
  constexpr uint32_t GLOG = dt_log2(GB);
  using G = typename DtGranule<GB>::type;
  using GG = __attribute__((address_space(1))) G;
  constexpr int U = DtUnroll<P, W>::value;
  constexpr int Q = NumOut<KIND, P>::value;
  // fewer than 2^32 granules per launch: q stays in 64 bits, q0 + q below 2^32 where q < nq
  const uint64_t t0 = (uint64_t)blockIdx.x * (kThreads * U) + threadIdx.x;
  uint64_t off[U];
  G x[U][P];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const uint64_t q = t0 + (uint64_t)u * kThreads;
    if (q < a.nq) {
      off[u] = reduce_dt_offset(a.lay, a.q0 + (uint32_t)q, GLOG);
#pragma unroll
      for (int p = 0; p < P; p++) x[u][p] = *(const GG*)((uint64_t)(uintptr_t)a.in[p] + off[u]);
    }
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    const uint64_t q = t0 + (uint64_t)u * kThreads;
    if (q < a.nq) {
      T e[P][W], r[Q][W];
#pragma unroll
      for (int p = 0; p < P; p++) __builtin_memcpy(e[p], &x[u][p], GB);
#pragma unroll
      for (int w = 0; w < W; w++) {
        T col[P], out[Q];
#pragma unroll
        for (int p = 0; p < P; p++) col[p] = e[p][w];
        eval_elem<F, P, KIND>(col, out, a.root);
#pragma unroll
        for (int k = 0; k < Q; k++) r[k][w] = out[k];
      }
      if constexpr (KIND == K_SCAN) {
#pragma unroll
        for (int k = 0; k < Q; k++) {
          G y;
          __builtin_memcpy(&y, r[k], GB);
          *(GG*)((uint64_t)(uintptr_t)a.out[k] + off[u]) = y;
        }
      } else {
        G y;
        __builtin_memcpy(&y, r[0], GB);
        for (int k = 0; k < a.nrep; k++) *(GG*)((uint64_t)(uintptr_t)a.out[k] + off[u]) = y;
      }
    }
  }
}

template <class F, int P, int KIND>
inline hipError_t launch_pw_dt(const PwayDtArgs& a, hipStream_t s, bool vec) {
  using T = typename F::T;
  constexpr int VW = 16 / (int)sizeof(T);
  if (a.nq == 0) return hipSuccess;
  auto grid = [&](int u) { return dim3((unsigned)(((uint64_t)a.nq + kThreads * u - 1) / (kThreads * u))); };
  if (vec && VW > 1) {
    hipLaunchKernelGGL((k_pway_dt<F, P, KIND, VW>), grid(DtUnroll<P, VW>::value), dim3(kThreads), 0, s, a);
  } else {  // one element per granule (a 16-B element is its own vector)
    hipLaunchKernelGGL((k_pway_dt<F, P, KIND, 1>), grid(DtUnroll<P, 1>::value), dim3(kThreads), 0, s, a);
  }
  return hipGetLastError();
}

// Every kind and P of one functor: K_FOLD P = 2..8, K_MST P = 3..8, K_SCAN P = 2..8. hipErrorInvalidValue otherwise.
template <class F>
inline hipError_t launch_functor_dt(int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec) {
  switch (kind) {
    case K_FOLD:
      switch (P) {
        case 2: return launch_pw_dt<F, 2, K_FOLD>(a, s, vec);
        case 3: return launch_pw_dt<F, 3, K_FOLD>(a, s, vec);
        case 4: return launch_pw_dt<F, 4, K_FOLD>(a, s, vec);
        case 5: return launch_pw_dt<F, 5, K_FOLD>(a, s, vec);
        case 6: return launch_pw_dt<F, 6, K_FOLD>(a, s, vec);
        case 7: return launch_pw_dt<F, 7, K_FOLD>(a, s, vec);
        case 8: return launch_pw_dt<F, 8, K_FOLD>(a, s, vec);
      }
      break;
    case K_MST:
      switch (P) {
        case 3: return launch_pw_dt<F, 3, K_MST>(a, s, vec);
        case 4: return launch_pw_dt<F, 4, K_MST>(a, s, vec);
        case 5: return launch_pw_dt<F, 5, K_MST>(a, s, vec);
        case 6: return launch_pw_dt<F, 6, K_MST>(a, s, vec);
        case 7: return launch_pw_dt<F, 7, K_MST>(a, s, vec);
        case 8: return launch_pw_dt<F, 8, K_MST>(a, s, vec);
      }
      break;
    case K_SCAN:
      switch (P) {
        case 2: return launch_pw_dt<F, 2, K_SCAN>(a, s, vec);
        case 3: return launch_pw_dt<F, 3, K_SCAN>(a, s, vec);
        case 4: return launch_pw_dt<F, 4, K_SCAN>(a, s, vec);
        case 5: return launch_pw_dt<F, 5, K_SCAN>(a, s, vec);
        case 6: return launch_pw_dt<F, 6, K_SCAN>(a, s, vec);
        case 7: return launch_pw_dt<F, 7, K_SCAN>(a, s, vec);
        case 8: return launch_pw_dt<F, 8, K_SCAN>(a, s, vec);
      }
      break;
  }
  return hipErrorInvalidValue;
}

// Implemented per op family in mpjx_k_dt_<family>.hip (split for parallel compilation). `type` is the base
// code (1..8), or 0x100 | base for the pair types of MAXLOC / MINLOC. `vec`: a.lay is in 16-B granules.
hipError_t launch_sum_dt(int type, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec);
hipError_t launch_prod_dt(int type, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec);
hipError_t launch_max_dt(int type, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec);
hipError_t launch_min_dt(int type, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec);
hipError_t launch_band_dt(int type, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec);
hipError_t launch_bor_dt(int type, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec);
hipError_t launch_bxor_dt(int type, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec);
hipError_t launch_logical_dt(int op, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec);
hipError_t launch_maxloc_dt(int type, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec);
hipError_t launch_minloc_dt(int type, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec);
// The dispatch over the op (mpjx_k_dt_dispatch.hip)
hipError_t launch_op_dt(int op, int type, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec);

}  // namespace mpjx
