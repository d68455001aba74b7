"""GPU: Datatype.Struct and resized types through each family of calls once (tests/struct_cases.py): Alltoall as the
distributed transpose at P = 2 and 3 multicore rank threads, checked against numpy on every rank; Scatterv and
Gatherv of column panels; Bcast of a Struct with a gap; Allreduce(SUM, DOUBLE) on resized columns at P = 2, bit for
bit the contiguous call on the packed vectors; Pack -> Unpack of a Struct, whose image equals the Hindexed type's with
the same blocks; and all of it at P = 2 over the RCCL stand-in, where the exchange engines pack and unpack. Whole
buffers are compared, gaps included."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import struct_cases as ST
from mpjexpress_amd import _lib
from mpjexpress_amd.mpi import MPI, Datatype, MPIException
from test_gpu_strided import free, run_ranks, world

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SO = os.path.join(ROOT, "tests", "rccl", "libmpjx_rccl_standin.so")
K_MOVES, K_STRIDED, K_INDEXED, K_TRANSPOSE = 1, 2, 4, 8


def kernels(comm):
    m = ctypes.c_uint(99)
    _lib.call("mpjx_comm_last_move_kernels", comm.handle, ctypes.byref(m))
    return m.value


def in_world(P, fn):
    comms = world(P)
    try:
        out, err = run_ranks(comms, lambda c: fn(torch, c, P))
    finally:
        free(comms)
    assert not any(err), err
    return out


@pytest.mark.parametrize("P", (1, 2, 3))
def test_alltoall_is_the_distributed_transpose(P):
    comms = world(P)
    try:
        out, err = run_ranks(comms, lambda c: (ST.alltoall_transpose(torch, c, P), kernels(c)))
    finally:
        free(comms)
    assert not any(err), err
    for r, (bad, mask) in enumerate(out):
        assert not bad, bad
        assert mask == (K_TRANSPOSE if r == 0 else 0), (r, mask)  # rank 0 launches for the world


@pytest.mark.parametrize("P", (1, 2, 3))
def test_scatter_and_gather_of_column_panels(P):
    for bad in in_world(P, ST.scatter_gather_panels):
        assert not bad, bad


@pytest.mark.parametrize("P", (1, 3))
def test_bcast_of_a_struct_with_a_gap(P):
    for bad in in_world(P, ST.bcast_struct):
        assert not bad, bad


@pytest.mark.parametrize("P", (1, 2))
def test_allreduce_on_resized_columns_equals_the_contiguous_call(P):
    for bad in in_world(P, ST.allreduce_column):
        assert not bad, bad


def test_pack_and_unpack_of_a_struct():
    for bad in in_world(1, ST.pack_round_trip):
        assert not bad, bad


def test_extent_zero_sends_and_is_refused_as_a_receive_type():
    comms = world(1)
    c = comms[0]
    z = Datatype.Struct([2, 1], [3, 3], [MPI.DOUBLE, MPI.UB])  # two doubles at 3, extent 0
    try:
        assert (z.Size(), z.Extent(), z.Lb(), z.Ub()) == (2, 0, 3, 3)
        src = np.arange(8, dtype=np.float64)
        s = torch.from_numpy(src).cuda()
        r = torch.full((8,), ST.SENT, dtype=torch.float64, device="cuda")
        c.Alltoall(s, 0, 3, z, r, 1, 6, MPI.DOUBLE)  # three items, every one the same two elements
        torch.cuda.synchronize()
        exp = np.full(8, ST.SENT)
        exp[1:7] = [3, 4, 3, 4, 3, 4]
        assert np.array_equal(r.cpu().numpy(), exp)
        c.Alltoall(s, 0, 2, MPI.DOUBLE, r, 0, 1, z)  # one item is a receive type like any other
        torch.cuda.synchronize()
        exp[3:5] = src[:2]
        assert np.array_equal(r.cpu().numpy(), exp)
        with pytest.raises(MPIException, match=r"\(-1\).*overlap"):  # last: a failed call fails its world
            c.Alltoall(s, 0, 6, MPI.DOUBLE, r, 0, 3, z)
        torch.cuda.synchronize()
        assert np.array_equal(r.cpu().numpy(), exp)  # refused before anything moved
    finally:
        z.Free()
        free(comms)


@pytest.mark.skipif(not os.path.exists(SO), reason="tests/rccl/libmpjx_rccl_standin.so is not built")
def test_every_family_over_rccl_transport_through_the_standin():
    env = dict(os.environ, MPJX_LIB_PATH=SO, RSI_TIMEOUT_S="30", MPJX_RCCL_TIMEOUT_S="30")
    env.pop("MPJX_TRANSPOSE", None)
    r = subprocess.run([sys.executable, "-u", os.path.join(ROOT, "tests", "struct_driver.py"), "rccl", "2"],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    d = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(d, indent=1))
    assert not d["bad"] and d["cases"] == len(ST.FAMILIES), d
    assert d["calls"].get("Group", 0) > 0, d["calls"]  # the exchanges ran
    assert "error" not in d["calls"], d["calls"]
    # every rank packed its own columns through k_transpose: the own block and the peer's pack in one launch
    assert all(m & K_TRANSPOSE for m in d["kernels"][0]), d["kernels"]
