// mpjx_k_dt_minloc.hip — k_pway_dt instantiations for the MINLOC functors (one op family per translation unit, as
// mpjx_k_minloc.hip). Type codes are mpi.Datatype base types (src/mpi/Datatype.java:57-66), 0x100 | base for the pairs.
#include "mpjx_kernels_dt.hpp"

namespace mpjx {
hipError_t launch_minloc_dt(int type, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec) {
  switch (type) {
    case 0x103: /* SHORT2 */ return launch_functor_dt<Minloc<int16_t>>(kind, P, a, s, vec);
    case 0x105: /* INT2 */ return launch_functor_dt<Minloc<int32_t>>(kind, P, a, s, vec);
    case 0x106: /* LONG2 */ return launch_functor_dt<Minloc<int64_t>>(kind, P, a, s, vec);
    case 0x107: /* FLOAT2 */ return launch_functor_dt<Minloc<float>>(kind, P, a, s, vec);
    case 0x108: /* DOUBLE2 */ return launch_functor_dt<Minloc<double>>(kind, P, a, s, vec);
  }
  return hipErrorInvalidValue;
}

}  // namespace mpjx
