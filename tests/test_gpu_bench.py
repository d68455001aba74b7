"""GPU: bench.py's N > 1 flow end to end on the one-GPU box, started the way a launcher-less driver
would start it (VERDICT r4 "do this" #1 and #2) — so every round's GPU test run also rehearses the
path the 8-GPU SCALE run takes:

- `python bench.py --launch --allreduce` — the parent starts `torch.distributed.run` itself (world of
  one), touching no GPU first; the child runs the preflights, every engine, and configs[0]/[3]/[4] with
  full parity; one JSON line with the launcher and budget records comes back;
- `python bench.py --gpus 2 --one-device` — two self-launched rank processes on the one GPU (IPC
  engines), `n_gpus` 2, bit-exact.
"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _bench(args, timeout=420):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
              "MPJX_BENCH_LAUNCHED"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, timeout=timeout, env=env,
                       cwd=ROOT)
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-1500:], r.stderr[-3000:])
    return json.loads(lines[0])


def _engines_exact(d):
    ran = {k: v for k, v in d["engines"].items() if "ms" in v}
    assert ran, d["engines"]
    for k, v in ran.items():
        assert v["mismatches"] == 0 and v["full_checksum_match"] is True, (k, v)
    return ran


@pytest.mark.gpu
def test_bench_plain_run_is_the_headline_only_and_dumps_its_last_recv(tmp_path):
    """A plain N = 1 run measures the headline only (nothing that --full adds is in the line), --steps
    sets the timed steps, and --dump-outputs writes the last timed step's recv: at P = 1 the send stream
    of pair (warmup + steps - 1) % sets, bit for bit (8 MiB: kept whole)."""
    import numpy as np

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import synth

    out = tmp_path / "dump"
    d = _bench(["--gpus", "1", "--steps", "4", "--warmup", "2", "--mib", "8", "--dump-outputs", str(out)], timeout=120)
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["full"] is False
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["parity"]["bit_exact"] is True
    assert d["unit"] == "GB/s" and d["dtype"] == "f64" and d["higher_is_better"] is True
    # value = S / t and ms_per_step = t, each rounded (2 and 4 decimals): equal within those roundings
    assert abs(d["value"] - (8 << 20) / (d["ms_per_step"] * 1e-3) / 1e9) <= d["value"] * 1e-4 / d["ms_per_step"] + 0.01
    for k in ("combine", "cpu_baseline", "configs0_multicore_p4"):
        assert k not in d, k
    assert "measured_copy_GBps" not in d["roofline"]
    assert sorted(os.listdir(out)) == ["allreduce_recv.npy"]
    got = np.load(out / "allreduce_recv.npy")
    n = (8 << 20) // 8
    exp = synth.uniform_np(np.arange(n, dtype=np.uint64), synth.seed(3, (2 + 4 - 1) % d["config"]["sets"]))
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), exp.view(np.uint64))


@pytest.mark.gpu
def test_bench_self_launched_world1_rehearsal():
    d = _bench(["--launch", "--allreduce", "--steps", "3", "--warmup", "1", "--no-variants", "--budget-s", "200"])
    assert d["n_gpus"] == 1 and d["value"] > 0 and d["parity"]["bit_exact"] is True, d.get("parity")
    rec = d["launcher"]
    assert rec["self_launched"] and "--nproc-per-node=1" in rec["cmd"]
    assert rec["parent_before_spawn"] == {"torch_imported": False, "hip_runtime_loaded": False,
                                          "gpu_device_open": False}
    ran = _engines_exact(d)
    assert {"rccl", "ipc"} <= set(ran), sorted(ran)
    assert "preflight:rccl" in d["budget"]["phase_wall_s"] and d["budget"]["skipped_for_budget"] == []
    assert all(v["ok"] for v in d["rccl_preflight"].values()), d["rccl_preflight"]


@pytest.mark.gpu
def test_bench_self_launched_two_ranks_one_device():
    d = _bench(["--gpus", "2", "--one-device", "--steps", "3", "--warmup", "1", "--no-variants"])
    assert d["n_gpus"] == 2 and d["parity"]["bit_exact"] is True, d.get("parity")
    assert d["launcher"]["self_launched"] and "--nproc-per-node=2" in d["launcher"]["cmd"]
    ran = _engines_exact(d)
    assert set(ran) <= {"ipc", "ipc_pull", "ipc_dsync"} and ran, sorted(ran)


@pytest.mark.gpu
def test_bench_world1_rccl_native_is_a_variant_not_the_engine():
    """RCCL's own reduction (MPJX_RCCL_NATIVE=1, one ncclAllReduce) is timed beside the
    reported engine as the comparison variant `rccl_native` (on a communicator of its own: the routing is
    read at init), never reported as the line's engine; the reported engine is one of libmpjx's
    HIP-combine engines. World-1 self-launched rehearsal with the comparison variants on."""
    d = _bench(["--launch", "--allreduce", "--full", "--steps", "3", "--warmup", "1", "--budget-s", "300"],
               timeout=600)
    import bench

    assert d["config"]["engine"] in bench.HEADLINE_ENGINES and "rccl_native" not in d["engines"], d["config"]
    v = d["variants"]["rccl_native"]
    assert v.get("bit_exact") is True and v.get("env") == {"MPJX_RCCL_NATIVE": "1"}, v
    assert "never the reported value" in v["note"]
    assert d["rccl_preflight"]["rccl_native"]["ok"], d["rccl_preflight"]
    assert d["variants"]["rccl_p2p"].get("bit_exact") is True, d["variants"].get("rccl_p2p")
