"""GPU: the reductions on derived datatypes in the worlds that have no direct engine for them, each in child
processes with its own time limit: RcclTransport at P = 2 and 3 through the RCCL stand-in build
(tests/reduce_dt_driver.py, rank threads on one GPU) and one IPC world of 2 rank processes with the shared-GPU
opt-in the other IPC tests use (tests/reduce_dt_ipc_worker.py). Each runs Allreduce, Reduce, Reduce_scatter and
Scan on one Vector type and one Indexed type, asserts the pack form and compares whole receive buffers."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SO = os.path.join(ROOT, "tests", "rccl", "libmpjx_rccl_standin.so")
LIMIT_S = 120

pytestmark = pytest.mark.gpu


def test_over_rccl_transport_through_the_standin():
    if not os.path.exists(SO):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "mpjexpress_amd"), "tests"])
    env = dict(os.environ, MPJX_LIB_PATH=SO, RSI_TIMEOUT_S="30", MPJX_RCCL_TIMEOUT_S="30")
    r = subprocess.run([sys.executable, "-u", os.path.join(HERE, "reduce_dt_driver.py"), "rccl", "2,3"],
                       capture_output=True, text=True, timeout=LIMIT_S, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert not d["bad"] and d["cases"] == 2 * 8, d
    assert sum(v for k, v in d["calls"].items() if k != "error") > 0, d["calls"]  # the transport's exchanges ran
    assert "error" not in d["calls"], d["calls"]


def test_in_an_ipc_world_of_two():
    P = 2
    uid = os.urandom(128).hex()
    env = dict(os.environ, MPJX_IPC_OVERSUBSCRIBE="1", MPJX_IPC_TIMEOUT_S="60")
    env.pop("MPJX_LIB_PATH", None)
    procs = [subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "reduce_dt_ipc_worker.py"), str(r), str(P), uid],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env) for r in range(P)]
    outs = []
    try:
        for p in procs:
            outs.append(p.communicate(timeout=LIMIT_S)[0])
    except subprocess.TimeoutExpired:
        for p in procs:
            p.kill()
        tails = [p.communicate()[0][-1500:] for p in procs]
        raise AssertionError(f"P={P} rank processes still running after {LIMIT_S} s:\n" + "\n---\n".join(tails))
    for r, (p, out) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, (r, out[-3000:])
        d = json.loads(out.strip().splitlines()[-1])
        assert d["rank"] == r and d["cases"] == 8 and not d["bad"], d
