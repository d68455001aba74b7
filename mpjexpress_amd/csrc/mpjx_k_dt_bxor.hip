// mpjx_k_dt_bxor.hip — k_pway_dt instantiations for the BXOR functors (one op family per translation unit, as
// mpjx_k_bxor.hip). Type codes are mpi.Datatype base types (src/mpi/Datatype.java:57-66).
#include "mpjx_kernels_dt.hpp"

namespace mpjx {
hipError_t launch_bxor_dt(int type, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec) {
  switch (type) {
    case 1: /* BYTE */ return launch_functor_dt<Bxor<uint8_t>>(kind, P, a, s, vec);
    case 2: /* CHAR */ return launch_functor_dt<Bxor<uint16_t>>(kind, P, a, s, vec);
    case 3: /* SHORT */ return launch_functor_dt<Bxor<uint16_t>>(kind, P, a, s, vec);
    case 5: /* INT */ return launch_functor_dt<Bxor<uint32_t>>(kind, P, a, s, vec);
    case 6: /* LONG */ return launch_functor_dt<Bxor<uint64_t>>(kind, P, a, s, vec);
  }
  return hipErrorInvalidValue;
}

}  // namespace mpjx
