// mpjx_k_dt_max.hip — k_pway_dt instantiations for the MAX functors (one op family per translation unit, as
// mpjx_k_max.hip). Type codes are mpi.Datatype base types (src/mpi/Datatype.java:57-66).
#include "mpjx_kernels_dt.hpp"

namespace mpjx {
hipError_t launch_max_dt(int type, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec) {
  switch (type) {
    case 1: /* BYTE */ return launch_functor_dt<Max<int8_t>>(kind, P, a, s, vec);
    case 2: /* CHAR */ return launch_functor_dt<Max<uint16_t>>(kind, P, a, s, vec);
    case 3: /* SHORT */ return launch_functor_dt<Max<int16_t>>(kind, P, a, s, vec);
    case 5: /* INT */ return launch_functor_dt<Max<int32_t>>(kind, P, a, s, vec);
    case 6: /* LONG */ return launch_functor_dt<Max<int64_t>>(kind, P, a, s, vec);
    case 7: /* FLOAT */ return launch_functor_dt<Max<float>>(kind, P, a, s, vec);
    case 8: /* DOUBLE */ return launch_functor_dt<Max<double>>(kind, P, a, s, vec);
  }
  return hipErrorInvalidValue;
}

}  // namespace mpjx
