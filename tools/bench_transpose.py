"""Time the transposed moves (k_transpose, mpjx_alltoallv_dt with a column type resized to one element) against
the same call on k_strided and the two things a caller runs without either, in ONE process, the variants of each row
interleaved repeat by repeat (tools/bench_strided.py's method: other work shares the host).

  python tools/bench_transpose.py [--mib 256,64] [--elems 4,8,16] [--iters 10] [--repeats 7] [--rotate 3]
                                  [--t-iters 200] [--skip-world]

Per row (--mib MiB packed; an element of 4, 8 or 16 bytes: INT, DOUBLE, DOUBLE2; a square N x N matrix; P = 1),
gather (N resized columns -> contiguous: the transpose lands packed) and scatter (contiguous -> N resized columns):
  transpose   mpjx_alltoallv_dt, the segment on k_transpose
  strided     the same call with MPJX_TRANSPOSE=0 (read per call): k_strided on the identical type
  torch       dst.copy_(src.t()): the pass a caller makes today before or after a contiguous move
  floor       k_moves on the same number of contiguous bytes (mpjx_allgather at P = 1)
--rotate R cycles every variant over R buffer sets, so no launch finds its operands in the 256 MiB Infinity Cache
from the one before (cold operands). Times are HIP events on the call's stream. mpjx_comm_last_move_kernels is
asserted for the two library variants, and the result is compared with torch's once per row.
world   P = 4 rank threads on one device, 1 MiB per rank pair: Alltoall with the resized column send type and a
        contiguous receive type (the distributed transpose in one call) against torch's transpose of the panels
        followed by mpjx_alltoall, each followed by mpjx_comm_synchronize; host clock of rank 0, --t-iters calls
        per repeat.
One JSON line per variant: every repeat's us, min, median, max; a summary line per row with the ratios and, for
each pair of variants, whether the gap of the medians is outside both spreads (max - min).
"""
import argparse
import ctypes
import json
import math
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

ELEMS = {4: (MPI.INT, torch.int32, 1), 8: (MPI.DOUBLE, torch.int64, 1), 16: (MPI.DOUBLE2, torch.int64, 2)}
K_STRIDED, K_TRANSPOSE = 2, 8


def report(name, us, **kw):
    r = dict(case=name, us=[round(x, 2) for x in us], min=round(min(us), 2), median=round(statistics.median(us), 2),
             max=round(max(us), 2), **kw)
    print(json.dumps(r), flush=True)
    return r


def i64(x):
    return (ctypes.c_int64 * 1)(x)


def column(rows, ld, old):
    v = Datatype.Vector(rows, 1, ld, old)
    t = Datatype.Struct([1, 1], [0, old.size], [v, MPI.UB])
    v.Free()
    return t


def gap(a, b):
    """'outside' if the medians of a and b differ by more than both spreads, else 'inside'."""
    d = abs(a["median"] - b["median"])
    return "outside both spreads" if d > a["max"] - a["min"] and d > b["max"] - b["min"] else "inside a spread"


def kernels(L, h):
    m = ctypes.c_uint()
    _lib.check(L.mpjx_comm_last_move_kernels(h, ctypes.byref(m)), "mpjx_comm_last_move_kernels")
    return m.value


def one_rank(a):
    L = _lib.lib()
    comm = mpi.smp_world(1, [0])[0]
    h = comm.handle
    st = torch.cuda.Stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    R = max(1, a.rotate)
    for mib in a.mib:
        for esz in a.elems:
            old, tdt, per = ELEMS[esz]
            N = int(math.isqrt((mib << 20) // esz)) // 16 * 16
            nbytes = N * N * esz
            words = N * N * per  # elements of the torch dtype
            shape = (N, N, per) if per > 1 else (N, N)
            mat = [torch.randint(0, 1 << 30, (words,), dtype=tdt, device="cuda") for _ in range(R)]
            flat = [torch.randint(0, 1 << 30, (words,), dtype=tdt, device="cuda") for _ in range(R)]
            col = column(N, N, old)
            base = old.baseType

            def gather(k):
                _lib.check(L.mpjx_alltoallv_dt(h, mat[k].data_ptr(), i64(N), i64(0), col.code, flat[k].data_ptr(),
                                               i64(N * N), i64(0), old.code, sp), "mpjx_alltoallv_dt")

            def scatter(k):
                _lib.check(L.mpjx_alltoallv_dt(h, flat[k].data_ptr(), i64(N * N), i64(0), old.code, mat[k].data_ptr(),
                                               i64(N), i64(0), col.code, sp), "mpjx_alltoallv_dt")

            def floor(k):
                _lib.check(L.mpjx_allgather(h, mat[k].data_ptr(), flat[k].data_ptr(), N * N * per, base, sp), "mpjx_allgather")

            def torch_gather(k):
                with torch.cuda.stream(st):
                    flat[k].view(shape).copy_(mat[k].view(shape).transpose(0, 1))

            def torch_scatter(k):
                with torch.cuda.stream(st):
                    mat[k].view(shape).transpose(0, 1).copy_(flat[k].view(shape))

            def off(fn):
                def go(k):
                    os.environ["MPJX_TRANSPOSE"] = "0"
                    try:
                        fn(k)
                    finally:
                        del os.environ["MPJX_TRANSPOSE"]
                return go
            rows = {"gather": {"transpose": gather, "strided": off(gather), "torch": torch_gather, "floor": floor},
                    "scatter": {"transpose": scatter, "strided": off(scatter), "torch": torch_scatter, "floor": floor}}
            # the moves are right at the sizes timed, on the kernel the column says
            for name, want in (("transpose", K_TRANSPOSE), ("strided", K_STRIDED)):
                src = mat[0].clone()
                torch.cuda.synchronize()
                rows["gather"][name](0)
                torch.cuda.synchronize()
                assert kernels(L, h) == want, (name, kernels(L, h))
                assert torch.equal(flat[0].view(shape), src.view(shape).transpose(0, 1)), f"gather {name} differs"
                mat[0].zero_()
                torch.cuda.synchronize()  # zero_ runs on torch's stream, the move on `st`
                rows["scatter"][name](0)
                torch.cuda.synchronize()
                assert kernels(L, h) == want, (name, kernels(L, h))
                assert torch.equal(mat[0], src), f"scatter {name} differs"
            for direction, variants in rows.items():
                for go in variants.values():  # warm
                    for k in range(max(2, R)):
                        go(k)
                torch.cuda.synchronize()
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
                out = {}
                for name, us in times.items():
                    med = statistics.median(us)
                    out[name] = report(f"{mib}MiB_{esz}B_{direction}_{name}", us, MiB=mib, elem_bytes=esz, N=N, rotate=R,
                                       iters=a.iters, bytes_moved=nbytes, GBps_moved=round(2 * nbytes / med / 1e3, 1))
                m = {k: v["median"] for k, v in out.items()}
                print(json.dumps({"case": f"{mib}MiB_{esz}B_{direction}_summary", "N": N,
                                  "transpose_over_floor": round(m["transpose"] / m["floor"], 3),
                                  "strided_over_floor": round(m["strided"] / m["floor"], 3),
                                  "torch_over_floor": round(m["torch"] / m["floor"], 3),
                                  "strided_over_transpose": round(m["strided"] / m["transpose"], 3),
                                  "torch_over_transpose": round(m["torch"] / m["transpose"], 3),
                                  "transpose_vs_strided": gap(out["transpose"], out["strided"]),
                                  "transpose_vs_torch": gap(out["transpose"], out["torch"]),
                                  "transpose_vs_floor": gap(out["transpose"], out["floor"])}), flush=True)
            col.Free()
            del mat, flat
    comm.Free()


def world_row(a, P=4):
    L = _lib.lib()
    comms = mpi.smp_world(P, [0] * P)
    rows, k = 256, 512  # a panel: 256 rows x 512 columns of doubles = 1 MiB per rank pair
    N = P * k
    blk = rows * k
    panel = [torch.randint(0, 1 << 40, (rows, N), dtype=torch.int64, device="cuda") for _ in range(P)]
    pack = [torch.empty(P * blk, dtype=torch.int64, device="cuda") for _ in range(P)]
    recv = [torch.empty(P * blk, dtype=torch.int64, device="cuda") for _ in range(P)]
    torch.cuda.synchronize()
    times = {"alltoall_resized_column": [], "torch_transpose_then_alltoall": []}
    masks = {}
    bar = threading.Barrier(P)
    arr = ctypes.c_int64 * P

    def body(r):
        torch.cuda.set_device(0)
        h = comms[r].handle
        col = column(rows, N, MPI.DOUBLE)
        sc, sd = arr(*[k] * P), arr(*[k * j for j in range(P)])
        rc, rd = arr(*[blk] * P), arr(*[blk * i for i in range(P)])

        def typed():
            _lib.check(L.mpjx_alltoallv_dt(h, panel[r].data_ptr(), sc, sd, col.code, recv[r].data_ptr(), rc, rd,
                                           MPI.DOUBLE.code, None), "mpjx_alltoallv_dt")
            _lib.check(L.mpjx_comm_synchronize(h), "sync")

        def packed():
            pack[r].view(P, k, rows).copy_(panel[r].view(rows, P, k).permute(1, 2, 0))
            torch.cuda.current_stream().synchronize()  # the mirrors synchronise the device before a call
            _lib.check(L.mpjx_alltoall(h, pack[r].data_ptr(), recv[r].data_ptr(), blk, MPI.DOUBLE.code, None), "mpjx_alltoall")
            _lib.check(L.mpjx_comm_synchronize(h), "sync")
        calls = {"alltoall_resized_column": typed, "torch_transpose_then_alltoall": packed}
        for rep in range(a.repeats + 1):  # repeat 0 warms both
            for name, call in calls.items():
                bar.wait(timeout=120)
                t0 = time.perf_counter()
                for _ in range(a.t_iters):
                    call()
                dt = (time.perf_counter() - t0) / a.t_iters * 1e6
                if r == 0 and rep > 0:
                    times[name].append(dt)
                if r == 0:
                    masks[name] = kernels(L, h)
                torch.cuda.synchronize()
                for i in range(P):  # either way: block i of rank r = the transpose of rank i's panel r
                    assert torch.equal(recv[r][i * blk:(i + 1) * blk].view(k, rows), panel[i][:, r * k:(r + 1) * k].t()), (name, r, i)
                recv[r].zero_()
                torch.cuda.synchronize()
        col.Free()
    th = [threading.Thread(target=body, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    out = {name: report(f"world_P{P}_{name}", us, P=P, pair_MiB=1, iters=a.t_iters, kernels=masks.get(name))
           for name, us in times.items()}
    x, y = out["alltoall_resized_column"], out["torch_transpose_then_alltoall"]
    print(json.dumps({"case": f"world_P{P}_summary", "torch_over_typed": round(y["median"] / x["median"], 3),
                      "typed_vs_torch": gap(x, y)}), flush=True)
    for c in comms:
        c.Free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=lambda s: [int(x) for x in s.split(",")], default=[256, 64])
    ap.add_argument("--elems", type=lambda s: [int(x) for x in s.split(",")], default=[4, 8, 16])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--t-iters", type=int, default=200)
    ap.add_argument("--skip-world", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    one_rank(a)
    if not a.skip_world:
        world_row(a)


if __name__ == "__main__":
    main()
