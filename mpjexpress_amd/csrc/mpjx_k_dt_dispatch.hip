// mpjx_k_dt_dispatch.hip — the dispatch of one k_pway_dt launch over the op; the kernel instantiations live in
// the mpjx_k_dt_<family>.hip files (compiled in parallel).
#include "mpjx_kernels_dt.hpp"

namespace mpjx {
hipError_t launch_op_dt(int op, int type, int kind, int P, const PwayDtArgs& a, hipStream_t s, bool vec) {
  switch (op) {
    case 1: return launch_max_dt(type, kind, P, a, s, vec);
    case 2: return launch_min_dt(type, kind, P, a, s, vec);
    case 3: return launch_sum_dt(type, kind, P, a, s, vec);
    case 4: return launch_prod_dt(type, kind, P, a, s, vec);
    case 5: case 7: case 9: return launch_logical_dt(op, kind, P, a, s, vec);
    case 6: return launch_band_dt(type, kind, P, a, s, vec);
    case 8: return launch_bor_dt(type, kind, P, a, s, vec);
    case 10: return launch_bxor_dt(type, kind, P, a, s, vec);
    case 11: return launch_maxloc_dt(type, kind, P, a, s, vec);
    case 12: return launch_minloc_dt(type, kind, P, a, s, vec);
  }
  return hipErrorInvalidValue;
}

}  // namespace mpjx
