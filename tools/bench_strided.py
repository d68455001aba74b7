"""Time the strided block-move kernel (k_strided, mpjx_alltoallv_dt) against the two things a caller runs
without it, in ONE process, the variants of each shape interleaved repeat by repeat (tools/bench_moves.py's
method: other work shares the host).

  python tools/bench_strided.py [--mib 256] [--iters 10] [--repeats 7] [--rotate 3] [--t-iters 200]
                                [--policies] [--skip-transpose]

Per shape (block bytes / stride bytes: 8/16, 128/256, 4096/8192; DOUBLE; --mib MiB packed; P = 1), gather
(Vector -> contiguous) and scatter (contiguous -> Vector):
  strided   mpjx_alltoallv_dt with a Vector on one side
  (a)       k_moves on the same number of contiguous bytes (mpjx_allgather, DOUBLE): the floor of a move
  (b)       torch's strided copy of the same shape (dst.copy_(src_view)): the pass a caller makes today before
            or after a contiguous move
--policies adds the strided kernel with its streaming threshold forced below and above the call
(MPJX_STRIDED_NT_MIN_MIB, read per call): the non-temporal form against the default-policy form on the same
bytes. --rotate R cycles every variant over R buffer sets, so no launch finds its operands in the 256 MiB
Infinity Cache from the one before (cold operands). Times are HIP events on the call's stream.
transpose   P = 4 rank threads on one device, a 1 MiB block per rank pair: Alltoallv with a Vector send type
            (256 rows of 4 KiB out of a 16 KiB-wide panel) against torch's pack of the same blocks followed by
            mpjx_alltoall, each followed by mpjx_comm_synchronize (the mirrors' blocking form); host clock of
            rank 0 per call.
One JSON line per variant: every repeat's us, min, median, max; bytes moved and bytes touched (whole 64-B
lines on the strided side).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from mpjexpress_amd import _lib, mpi  # noqa: E402
from mpjexpress_amd.mpi import MPI, Datatype  # noqa: E402

DOUBLE = 8
SHAPES = ((8, 16), (128, 256), (4096, 8192))


def report(name, us, **kw):
    r = dict(case=name, us=[round(x, 2) for x in us], min=round(min(us), 2), median=round(statistics.median(us), 2),
             max=round(max(us), 2), **kw)
    print(json.dumps(r), flush=True)
    return r


def i64(x):
    return (ctypes.c_int64 * 1)(x)


def one_rank(a):
    L = _lib.lib()
    comm = mpi.smp_world(1, [0])[0]
    h = comm.handle
    st = torch.cuda.Stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    nbytes = a.mib << 20
    n = nbytes // 8
    R = max(1, a.rotate)
    packed = [torch.randint(0, 1 << 40, (n,), dtype=torch.int64, device="cuda") for _ in range(R)]
    flat = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(R)]
    for bb, sb in SHAPES:
        bl, stl, nblocks = bb // 8, sb // 8, nbytes // bb
        vec = Datatype.Vector(nblocks, bl, stl, MPI.DOUBLE)
        wide = [torch.randint(0, 1 << 40, (nblocks * stl,), dtype=torch.int64, device="cuda") for _ in range(R)]

        def gather(k):
            _lib.check(L.mpjx_alltoallv_dt(h, wide[k].data_ptr(), i64(1), i64(0), vec.code, flat[k].data_ptr(), i64(n),
                                           i64(0), DOUBLE, sp), "mpjx_alltoallv_dt")

        def scatter(k):
            _lib.check(L.mpjx_alltoallv_dt(h, packed[k].data_ptr(), i64(n), i64(0), DOUBLE, wide[k].data_ptr(), i64(1),
                                           i64(0), vec.code, sp), "mpjx_alltoallv_dt")

        def contiguous(k):
            _lib.check(L.mpjx_allgather(h, packed[k].data_ptr(), flat[k].data_ptr(), n, DOUBLE, sp), "mpjx_allgather")

        def torch_gather(k):
            with torch.cuda.stream(st):
                flat[k].view(nblocks, bl).copy_(wide[k].view(nblocks, stl)[:, :bl])

        def torch_scatter(k):
            with torch.cuda.stream(st):
                wide[k].view(nblocks, stl)[:, :bl].copy_(packed[k].view(nblocks, bl))

        def forced(fn, mib):
            def go(k):
                os.environ["MPJX_STRIDED_NT_MIN_MIB"] = str(mib)
                try:
                    fn(k)
                finally:
                    del os.environ["MPJX_STRIDED_NT_MIN_MIB"]
            return go
        variants = {"gather_strided": gather, "scatter_strided": scatter, "a_k_moves_contiguous": contiguous,
                    "b_torch_gather": torch_gather, "b_torch_scatter": torch_scatter}
        if a.policies:
            variants.update({"gather_strided_nt": forced(gather, 1), "gather_strided_default": forced(gather, 1 << 20),
                             "scatter_strided_nt": forced(scatter, 1), "scatter_strided_default": forced(scatter, 1 << 20)})
        for go in variants.values():  # warm every shape
            for k in range(max(2, R)):
                go(k)
        torch.cuda.synchronize()
        # the moves are right at the sizes timed
        gather(0)
        torch.cuda.synchronize()
        assert torch.equal(flat[0].view(nblocks, bl), wide[0].view(nblocks, stl)[:, :bl]), "gather differs"
        keep = wide[0].view(nblocks, stl)[:, bl:].clone()
        scatter(0)
        torch.cuda.synchronize()
        assert torch.equal(wide[0].view(nblocks, stl)[:, :bl], packed[0].view(nblocks, bl)), "scatter differs"
        assert torch.equal(wide[0].view(nblocks, stl)[:, bl:], keep), "scatter wrote into a gap"
        del keep
        times = {k: [] for k in variants}
        for _ in range(a.repeats):
            for name, go in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                for k in range(a.iters):
                    go(k % R)
                e1.record(st)
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / a.iters * 1e3)
        lines = 64 * -(-bb // 64) * nblocks if sb >= 64 else nblocks * sb  # whole 64-B lines under the blocks
        out = {}
        for name, us in times.items():
            touched = 2 * nbytes if name.startswith("a_") else nbytes + lines
            med = statistics.median(us)
            out[name] = report(f"{bb}B_of_{sb}B_{name}", us, MiB=a.mib, rotate=R, iters=a.iters, block_bytes=bb,
                               stride_bytes=sb, bytes_moved=nbytes, bytes_touched=touched,
                               GBps_moved=round(2 * nbytes / med / 1e3, 1), GBps_touched=round(touched / med / 1e3, 1))
        m = {k: v["median"] for k, v in out.items()}
        spread = {k: round(v["max"] - v["min"], 2) for k, v in out.items()}
        print(json.dumps({"case": f"{bb}B_of_{sb}B_summary",
                          "gather_over_a": round(m["gather_strided"] / m["a_k_moves_contiguous"], 4),
                          "scatter_over_a": round(m["scatter_strided"] / m["a_k_moves_contiguous"], 4),
                          "gather_over_b": round(m["gather_strided"] / m["b_torch_gather"], 4),
                          "scatter_over_b": round(m["scatter_strided"] / m["b_torch_scatter"], 4),
                          "spread_us": spread}), flush=True)
        vec.Free()
        del wide
    comm.Free()


def transpose(a, P=4):
    L = _lib.lib()
    comms = mpi.smp_world(P, [0] * P)
    rows, bw = 256, 512  # a block: 256 rows of 512 doubles = 1 MiB
    N = P * bw
    blk = rows * bw
    panel = [torch.randint(0, 1 << 40, (rows, N), dtype=torch.int64, device="cuda") for _ in range(P)]
    pack = [torch.empty(P * blk, dtype=torch.int64, device="cuda") for _ in range(P)]
    recv = [torch.empty(P * blk, dtype=torch.int64, device="cuda") for _ in range(P)]
    torch.cuda.synchronize()
    times = {"alltoallv_vector": [], "torch_pack_then_alltoall": []}
    bar = threading.Barrier(P)
    arr = ctypes.c_int64 * P

    def body(r):
        torch.cuda.set_device(0)
        h = comms[r].handle
        block = Datatype.Vector(rows, bw, N, MPI.DOUBLE)
        sc, sd = arr(*[1] * P), arr(*[bw * j for j in range(P)])
        rc, rd = arr(*[blk] * P), arr(*[blk * i for i in range(P)])

        def vector():
            _lib.check(L.mpjx_alltoallv_dt(h, panel[r].data_ptr(), sc, sd, block.code, recv[r].data_ptr(), rc, rd, DOUBLE,
                                           None), "mpjx_alltoallv_dt")
            _lib.check(L.mpjx_comm_synchronize(h), "sync")

        def packed():
            pack[r].view(P, rows, bw).copy_(panel[r].view(rows, P, bw).permute(1, 0, 2))
            torch.cuda.current_stream().synchronize()  # the mirrors synchronise the device before a call
            _lib.check(L.mpjx_alltoall(h, pack[r].data_ptr(), recv[r].data_ptr(), blk, DOUBLE, None), "mpjx_alltoall")
            _lib.check(L.mpjx_comm_synchronize(h), "sync")
        calls = {"alltoallv_vector": vector, "torch_pack_then_alltoall": packed}
        for rep in range(a.repeats + 1):  # repeat 0 warms both
            for name, call in calls.items():
                bar.wait(timeout=120)
                t0 = time.perf_counter()
                for _ in range(a.t_iters):
                    call()
                dt = (time.perf_counter() - t0) / a.t_iters * 1e6
                if r == 0 and rep > 0:
                    times[name].append(dt)
                torch.cuda.synchronize()
                for i in range(P):  # either way: block i of rank r = rank i's columns of block r
                    assert torch.equal(recv[r][i * blk:(i + 1) * blk].view(rows, bw), panel[i][:, r * bw:(r + 1) * bw]), (name, r, i)
                recv[r].zero_()
                torch.cuda.synchronize()
        block.Free()
    th = [threading.Thread(target=body, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for name, us in times.items():
        report(f"transpose_P{P}_{name}", us, P=P, block_MiB=1, iters=a.t_iters)
    for c in comms:
        c.Free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--t-iters", type=int, default=200)
    ap.add_argument("--policies", action="store_true")
    ap.add_argument("--skip-transpose", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    one_rank(a)
    if not a.skip_transpose:
        transpose(a)


if __name__ == "__main__":
    main()
