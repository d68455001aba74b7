"""GPU: every k_pway_dt instantiation the library can launch, against the oracle. One test per (P in 2..8) x (op in
the 12 ops); within it every type valid for the op, at both granule widths where the type has two, through
  Allreduce, new collectives          K_MST at P >= 3, K_FOLD at P = 2
  Reduce, old collectives, root P - 1 K_FOLD at P >= 3 in the FT order
  Scan                                K_SCAN
which together reach every (functor, kind, P, W) of launch_functor_dt through the three levels of switch
statements that choose it (reduce_dt_cases.matrix_cases; tests/test_reduce_dt_case_power.py holds, on the CPU, that
the parametrisation covers all 2,160 such paths — 1,960 distinct kernels, SHORT and CHAR sharing the SUM, PROD, BAND,
BOR and BXOR functors — and that no case's result equals an operand). Every call must take the
direct form; whole buffers are compared byte for byte and the send buffers must come back unchanged. The launches
are one full tile and a partial one; one irregular layout per test takes the table search of reduce_dt_offset."""
import pytest

import oracle as O
import reduce_dt_cases as RC
from test_gpu_reduce_dt import run_world

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.mark.parametrize("op", RC.OPS, ids=[O.OP_NAMES[op] for op in RC.OPS])
@pytest.mark.parametrize("P", range(2, 9))
def test_every_instantiation(P, op):
    new, old = RC.matrix_cases(P, op)
    run_world(P, new, RC.FORM_DIRECT)
    run_world(P, old, RC.FORM_DIRECT, old=True)
