"""GPU: the block moves with irregular datatypes over RcclTransport at P = 2 and 3 on one GPU, through the RCCL stand-in build
(tests/rccl/libmpjx_rccl_standin.so) driven by tests/indexed_driver.py in a child process: irregular sends are
packed into communicator scratch, the packed bytes go through exchange (grouped ncclSend / ncclRecv), irregular
receives are unpacked; the rank's own block moves from layout to layout. All nine mirror methods with a
Indexed or Hindexed type on either side (tests/indexed_cases.py), INT and DOUBLE2, whole receive buffers compared byte for byte."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "rccl", "libmpjx_rccl_standin.so")


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(SO), reason="tests/rccl/libmpjx_rccl_standin.so is not built")
def test_indexed_moves_over_rccl_transport_through_the_standin():
    env = dict(os.environ, MPJX_LIB_PATH=SO, RSI_TIMEOUT_S="30", MPJX_RCCL_TIMEOUT_S="30")
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "indexed_driver.py"), "rccl", "2,3",
                        "INT,DOUBLE2"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    d = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(d, indent=1))
    assert not d["bad"] and d["cases"] == 2 * 2 * 42, d
    assert d["calls"].get("Group", 0) > 0, d["calls"]  # the exchanges ran
    assert "error" not in d["calls"], d["calls"]
