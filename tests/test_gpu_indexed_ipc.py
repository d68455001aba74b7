"""GPU: the block moves with irregular datatypes (tests/indexed_cases.py) in one IPC world of 2 rank processes on one GPU
(tests/indexed_ipc_worker.py): all nine mirror methods with an Indexed or Hindexed type on either side, rooted calls at both
roots, through pack -> IpcTransport::exchange -> unpack. One small world on purpose: the one-GPU stalls on
record were 8-process worlds."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LIMIT_S = 120


@pytest.mark.gpu
def test_nine_methods_in_an_ipc_world_of_two():
    P = 2
    uid = os.urandom(128).hex()
    env = dict(os.environ, MPJX_IPC_OVERSUBSCRIBE="1", MPJX_IPC_TIMEOUT_S="60")
    env.pop("MPJX_LIB_PATH", None)
    procs = [subprocess.Popen([sys.executable, "-u", os.path.join(HERE, "indexed_ipc_worker.py"), str(r), str(P), uid,
                               "INT"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
             for r in range(P)]
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
        assert d["rank"] == r and d["cases"] == 42 and not d["bad"], d
