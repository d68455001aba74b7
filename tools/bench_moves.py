"""Time the block-move kernel (k_moves) and the one-launch multicore engine against the parent paths, in
ONE process, the variants of each comparison interleaved repeat by repeat (other work shares the host).

  python tools/bench_moves.py [--mib 256] [--iters 20] [--repeats 7] [--rotate 3] [--a2a-iters 200]

aligned     P = 1 mpjx_allgather of --mib MiB DOUBLE (k_moves, streaming form) against P = 1
            mpjx_allreduce(SUM, DOUBLE) of the same bytes (Reduce = arraycopy: k_copies, the bench's headline
            operation). Same bytes, same access width.
misaligned  the same bytes as BYTE with the send pointer at +1 and the receive pointer at +2 (k_moves: two
            aligned 16-B loads and a byte shift per 16-B store) against the aligned figure, and against
            P = 1 mpjx_allreduce(SUM, BYTE) at the same pointers — which is NOT k_copies' byte-wise path:
            Combine::copy_o hands misaligned pairs to hipMemcpyAsync (mpjx_internal.hpp). k_copies' byte-wise
            path runs only inside IpcTransport::exchange and cannot be reached from one process.
alltoall    mpjx_alltoall, 1 MiB INT blocks, P = 4 and P = 8 rank threads on one device, each call followed by
            mpjx_comm_synchronize (the mirrors' blocking form): the one-launch engine against MPJX_SMP_COPY=1
            (SmpTransport::exchange, the parent's only way to move such blocks between device buffers).
--rotate R cycles the P = 1 cases over R buffer sets, so no launch finds its operands in the 256 MiB
Infinity Cache from the one before (cold operands, as bench_pway.py --rotate). Times are HIP events on the
call's stream (P = 1) or the host clock of rank 0 around blocking calls (alltoall). One JSON line per
variant: every repeat's us, min, median, max.
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

BYTE, INT, DOUBLE, SUM = 1, 5, 8, 3


def report(name, us, **kw):
    r = dict(case=name, us=[round(x, 2) for x in us], min=round(min(us), 2), median=round(statistics.median(us), 2),
             max=round(max(us), 2), **kw)
    print(json.dumps(r), flush=True)
    return r


def one_rank(a):
    L = _lib.lib()
    comm = mpi.smp_world(1, [0])[0]
    h = comm.handle
    st = torch.cuda.Stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    nbytes = a.mib << 20
    R = max(1, a.rotate)
    pad = 256
    src = [torch.randint(0, 256, (nbytes + pad,), dtype=torch.uint8, device="cuda") for _ in range(R)]
    dst = [torch.empty(nbytes + pad, dtype=torch.uint8, device="cuda") for _ in range(R)]
    nb = nbytes - 16  # the misaligned cases move 16 bytes less, inside the same buffers

    def variant(fn, count, type_, so, ro, *tail):
        def go(k):
            k %= R
            _lib.check(fn(h, src[k].data_ptr() + so, dst[k].data_ptr() + ro, count, type_, *tail, sp), fn.__name__)
        return go
    variants = {
        "aligned_k_moves_allgather_double": variant(L.mpjx_allgather, nbytes // 8, DOUBLE, 0, 0),
        "aligned_k_copies_allreduce_double": variant(L.mpjx_allreduce, nbytes // 8, DOUBLE, 0, 0, SUM, 0),
        "misaligned_k_moves_allgather_byte_s1_r2": variant(L.mpjx_allgather, nb, BYTE, 1, 2),
        "misaligned_memcpy_allreduce_byte_s1_r2": variant(L.mpjx_allreduce, nb, BYTE, 1, 2, SUM, 0),
    }
    for go in variants.values():  # warm every shape
        for k in range(max(3, R)):
            go(k)
    torch.cuda.synchronize()
    # the moves are right at the sizes timed
    variants["misaligned_k_moves_allgather_byte_s1_r2"](0)
    torch.cuda.synchronize()
    assert torch.equal(dst[0][2:2 + nb], src[0][1:1 + nb]), "misaligned move differs"
    variants["aligned_k_moves_allgather_double"](0)
    torch.cuda.synchronize()
    assert torch.equal(dst[0][:nbytes], src[0][:nbytes]), "aligned move differs"
    times = {k: [] for k in variants}
    for _ in range(a.repeats):
        for name, go in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            for k in range(a.iters):
                go(k)
            e1.record(st)
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / a.iters * 1e3)
    out = {}
    for name, us in times.items():
        moved = nbytes if name.startswith("aligned") else nb
        out[name] = report(name, us, MiB=a.mib, rotate=R, iters=a.iters, bytes_moved=moved,
                           GBps_at_median=round(2 * moved / statistics.median(us) / 1e3, 1))
    m = {k: v["median"] for k, v in out.items()}
    print(json.dumps({"case": "ratios_of_medians",
                      "k_moves_over_k_copies_aligned": round(m["aligned_k_moves_allgather_double"] /
                                                             m["aligned_k_copies_allreduce_double"], 4),
                      "k_moves_misaligned_over_aligned": round(m["misaligned_k_moves_allgather_byte_s1_r2"] /
                                                               m["aligned_k_moves_allgather_double"], 4),
                      "k_moves_misaligned_over_memcpy": round(m["misaligned_k_moves_allgather_byte_s1_r2"] /
                                                              m["misaligned_memcpy_allreduce_byte_s1_r2"], 4)}), flush=True)
    del src, dst
    comm.Free()


def alltoall(a, P):
    L = _lib.lib()
    comms = mpi.smp_world(P, [0] * P)
    n = (1 << 20) // 4  # 1 MiB INT blocks
    send = [torch.randint(0, 1 << 30, (n * P,), dtype=torch.int32, device="cuda") for _ in range(P)]
    recv = [torch.empty(n * P, dtype=torch.int32, device="cuda") for _ in range(P)]
    torch.cuda.synchronize()
    times = {"one_launch": [], "smp_copy_exchange": []}
    bar = threading.Barrier(P)

    def body(r):
        torch.cuda.set_device(0)
        h = comms[r].handle

        def call():
            _lib.check(L.mpjx_alltoall(h, send[r].data_ptr(), recv[r].data_ptr(), n, INT, None), "mpjx_alltoall")
            _lib.check(L.mpjx_comm_synchronize(h), "sync")
        for rep in range(a.repeats + 1):  # repeat 0 warms both engines
            for name in times:
                bar.wait()
                if r == 0:  # read per call by every rank: set between the barriers, while no call runs
                    if name == "smp_copy_exchange":
                        os.environ["MPJX_SMP_COPY"] = "1"
                    else:
                        os.environ.pop("MPJX_SMP_COPY", None)
                bar.wait()
                t0 = time.perf_counter()
                for _ in range(a.a2a_iters):
                    call()
                dt = (time.perf_counter() - t0) / a.a2a_iters * 1e6
                if r == 0 and rep > 0:
                    times[name].append(dt)
    th = [threading.Thread(target=body, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    os.environ.pop("MPJX_SMP_COPY", None)
    torch.cuda.synchronize()
    for r in range(P):  # the last engine's result: block i of rank r = block r of rank i
        for i in range(P):
            assert torch.equal(recv[r][i * n:(i + 1) * n], send[i][r * n:(r + 1) * n]), (r, i)
    for name, us in times.items():
        report(f"alltoall_P{P}_{name}", us, P=P, block_MiB=1, iters=a.a2a_iters)
    for c in comms:
        c.Free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--a2a-iters", type=int, default=200)
    ap.add_argument("--skip-alltoall", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    one_rank(a)
    if not a.skip_alltoall:
        for P in (4, 8):
            alltoall(a, P)


if __name__ == "__main__":
    main()
