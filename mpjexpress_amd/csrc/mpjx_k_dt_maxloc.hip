// mpjx_k_dt_maxloc.hip — k_pway_dt instantiations for the MAXLOC functors (one op family per translation unit, as
// mpjx_k_maxloc.hip). Type codes are mpi.Datatype base types (src/mpi/Datatype.java:57-66), 0x100 | base for the pairs.
#include "mpjx_kernels_dt.hpp"

namespace mpjx {
hipError_t launch_maxloc_dt(int type, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec) {
  switch (type) {
    case 0x103: /* SHORT2 */ return launch_functor_dt<Maxloc<int16_t>>(kind, P, a, s, vec);
    case 0x105: /* INT2 */ return launch_functor_dt<Maxloc<int32_t>>(kind, P, a, s, vec);
    case 0x106: /* LONG2 */ return launch_functor_dt<Maxloc<int64_t>>(kind, P, a, s, vec);
    case 0x107: /* FLOAT2 */ return launch_functor_dt<Maxloc<float>>(kind, P, a, s, vec);
    case 0x108: /* DOUBLE2 */ return launch_functor_dt<Maxloc<double>>(kind, P, a, s, vec);
  }
  return hipErrorInvalidValue;
}

}  // namespace mpjx
