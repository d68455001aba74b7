// mpjx_k_dt_logical.hip — k_pway_dt instantiations for the LAND / LOR / LXOR functors on BOOLEAN (one op family
// per translation unit, as mpjx_k_logical.hip; the faithful Keep functors have no derived-type form).
#include "mpjx_kernels_dt.hpp"

namespace mpjx {
hipError_t launch_logical_dt(int op, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec) {
  switch (op) {
    case 5: return launch_functor_dt<Land>(kind, P, a, s, vec);  /* LAND */
    case 7: return launch_functor_dt<Lor>(kind, P, a, s, vec);   /* LOR */
    case 9: return launch_functor_dt<Lxor>(kind, P, a, s, vec);  /* LXOR */
  }
  return hipErrorInvalidValue;
}

}  // namespace mpjx
