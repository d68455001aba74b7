"""Runs the reductions on derived datatypes (tests/reduce_dt_cases.py's child_cases) on rank threads in a fresh
process, over the RCCL stand-in build the caller names in MPJX_LIB_PATH (tests/test_gpu_reduce_dt_standin.py):

    python tests/reduce_dt_driver.py rccl P[,P...]

The worlds are tests/moves_driver.py's. RcclTransport has no direct engine, so every call must take the pack
path: pack -> the contiguous call over the transport's exchanges -> unpack. Prints one JSON line:
{"cases": n, "bad": [messages], "calls": {rccl call: count}}.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle"), HERE]

import torch  # noqa: E402

import moves_driver as MD  # noqa: E402
import reduce_dt_cases as RC  # noqa: E402
from mpjexpress_amd import _lib  # noqa: E402


def main():
    engine, Ps = sys.argv[1], [int(p) for p in sys.argv[2].split(",")]
    assert engine == "rccl", engine
    L = _lib.lib()
    assert L.rsi_is_standin() == 1, "MPJX_LIB_PATH does not name the stand-in build"
    bad, n = [], 0
    try:
        for P in Ps:
            comms = MD.rccl_world(P)
            cases = RC.child_cases(P)
            try:
                out = MD.threads(P, lambda r: RC.run_cases(torch, comms[r], cases, RC.FORM_PACK))
                bad += [m for res in out for m in res]
                n += len(cases)
            finally:
                MD.threads(P, lambda r: comms[r].Free())
    except BaseException as e:  # noqa: BLE001
        bad.append(f"raised {e!r}"[:2000])
    print(json.dumps({"cases": n, "bad": bad, "calls": MD.standin_calls(L)}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
