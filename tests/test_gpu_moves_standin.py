"""GPU: the block-move collectives over RcclTransport at P = 2, 3, 5 on one GPU, through the RCCL stand-in
build (tests/rccl/libmpjx_rccl_standin.so: the same libmpjx objects linked against tests/rccl/rccl_standin.hip)
driven by tests/moves_driver.py in a child process. Allgather goes through allgather_equal (the in-place
ncclAllGather), Alltoall(v) through alltoallv (ncclAllToAllv), Allgatherv / Gatherv / Scatterv through
exchange (grouped ncclSend / ncclRecv); the rank's own block is moved by k_moves. INT and BYTE, the
ragged matrix of tests/moves_cases.py, whole receive buffers compared byte for byte."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "rccl", "libmpjx_rccl_standin.so")


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(SO), reason="tests/rccl/libmpjx_rccl_standin.so is not built")
def test_block_moves_over_rccl_transport_through_the_standin():
    env = dict(os.environ, MPJX_LIB_PATH=SO, RSI_TIMEOUT_S="30", MPJX_RCCL_TIMEOUT_S="30")
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "moves_driver.py"), "rccl", "2,3,5",
                        "INT,BYTE"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    d = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(d, indent=1))
    assert not d["bad"] and d["cases"] == 3 * 2 * 8, d
    for call in ("AllGather", "AllToAllv", "Group"):
        assert d["calls"].get(call, 0) > 0, (call, d["calls"])
    assert "error" not in d["calls"], d["calls"]
