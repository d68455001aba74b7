"""Persistent-request timing: what Send_init / Recv_init once + Startall / Waitall per iteration costs beside
Isend / Irecv / Waitall per iteration, and whether the device segment pool (k_msgs_pool) earns its place.

  halo        the P = 4 halo exchange of tools/bench_p2p.py on 1024 x 1024 DOUBLE tiles (4 receives + 4 sends per
              rank: rows contiguous, columns Vector), from Python rank threads, three ways:
                isend        Isend / Irecv / Waitall every iteration (bench_p2p's "batched" row)
                persistent   the requests made once, then Startall / Waitall
                persistent, MPJX_P2P_POOL=0   the same with every batch on the table path
  neighbours  26 messages of 8 KiB per rank and iteration at P = 4 (a 3-D 26-neighbour halo folded onto four ranks:
              message k goes to rank (me + 1 + k % 3) % 4 under tag k), persistent, with the pool and with
              MPJX_P2P_POOL=0: up to 52 matched pairs per Waitall, which is three k_msgs tables or one index

  python tools/bench_preq.py [--iters 30] [--warmup 5] [--tile 1024] [--msg-bytes 8192] [--out FILE]

Times are host wall-clock per exchange on rank 0 (Startall + Waitall, or the posts + Waitall), the median over
--iters with the minimum and the maximum, on cold operands as tools/bench_p2p.py makes them: before every timed
exchange rank 0 rewrites a 512 MiB scratch buffer outside the timed region and the ranks meet at a barrier.
One JSON line per row."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_p2p import FLUSH_BYTES, run  # noqa: E402
from mpjexpress_amd import mpi  # noqa: E402
from mpjexpress_amd.mpi import MPI, Datatype, Prequest, Request  # noqa: E402


def world(P, pool):
    old = os.environ.pop("MPJX_P2P_POOL", None)
    if not pool:
        os.environ["MPJX_P2P_POOL"] = "0"  # read once, when the world is created
    try:
        return mpi.smp_world(P, [0] * P)
    finally:
        os.environ.pop("MPJX_P2P_POOL", None)
        if old is not None:
            os.environ["MPJX_P2P_POOL"] = old


def timed(c, flush, step, iters, warmup):
    """(median, min, max) seconds of step() over iters cold runs (this rank's clock; every rank runs step)."""
    ts = []
    for i in range(warmup + iters):
        if c.Rank() == 0:
            flush.add_(1)
            torch.cuda.synchronize()
        c.Barrier()
        t0 = time.perf_counter()
        step()
        t1 = time.perf_counter()
        if i >= warmup:
            ts.append(t1 - t0)
    return statistics.median(ts), min(ts), max(ts)


def row(bench, mode, sec, comms_stats, **kv):
    med, lo, hi = sec
    out = {"bench": bench, "mode": mode, "us": round(med * 1e6, 2), "us_min": round(lo * 1e6, 2), "us_max": round(hi * 1e6, 2)}
    out.update(kv)
    out.update(comms_stats)
    return out


def totals(rows):
    return {"launches_all_ranks": sum(r[0][0] for r in rows), "pool_launches_all_ranks": sum(r[1][0] for r in rows),
            "puts_all_ranks": sum(r[1][1] for r in rows), "hits_all_ranks": sum(r[1][2] for r in rows)}


def halo(a, mode, flush):
    comms = world(4, mode != "persistent_pool_off")
    T = a.tile
    N = T + 2
    col = Datatype.Vector(T, 1, N, MPI.DOUBLE)

    def body(c):
        me = c.Rank()
        i, j = divmod(me, 2)
        nb = {"n": ((i - 1) % 2) * 2 + j, "s": ((i + 1) % 2) * 2 + j, "w": i * 2 + (j - 1) % 2, "e": i * 2 + (j + 1) % 2}
        t = (torch.arange(N * N, dtype=torch.float64, device="cuda") + me * 1e7)
        at = lambda r, k: r * N + k  # noqa: E731

        def requests(recv, send):
            return [
                recv(t, at(N - 1, 1), T, MPI.DOUBLE, nb["s"], 0), recv(t, at(0, 1), T, MPI.DOUBLE, nb["n"], 1),
                recv(t, at(1, N - 1), 1, col, nb["e"], 2), recv(t, at(1, 0), 1, col, nb["w"], 3),
                send(t, at(1, 1), T, MPI.DOUBLE, nb["n"], 0), send(t, at(N - 2, 1), T, MPI.DOUBLE, nb["s"], 1),
                send(t, at(1, 1), 1, col, nb["w"], 2), send(t, at(1, N - 2), 1, col, nb["e"], 3),
            ]
        if mode == "isend":
            def step():
                Request.Waitall(requests(c.Irecv, c.Isend))
        else:
            req = requests(c.Recv_init, c.Send_init)

            def step():
                Prequest.Startall(req)
                Request.Waitall(req)
        sec = timed(c, flush, step, a.iters, a.warmup)
        return c.p2p_stats(), c.p2p_pool_stats(), sec
    rows = run(comms, body)
    col.Free()
    for c in comms:
        c.Free()
    return [row("halo", mode, rows[0][2], totals(rows), tile=T, bytes_per_rank=4 * T * 8)]


def neighbours(a, mode, flush):
    comms = world(4, mode != "persistent_pool_off")
    n, K = a.msg_bytes // 8, 26

    def body(c):
        me = c.Rank()
        s = torch.arange(K * n, dtype=torch.float64, device="cuda") + me * 1e7
        r = torch.zeros(K * n, dtype=torch.float64, device="cuda")
        req = []
        for k in range(K):  # the message I receive under tag k comes from the rank whose (peer + 1 + k % 3) % 4 is me
            req.append(c.Recv_init(r, k * n, n, MPI.DOUBLE, (me - 1 - k % 3) % 4, k))
        for k in range(K):
            req.append(c.Send_init(s, k * n, n, MPI.DOUBLE, (me + 1 + k % 3) % 4, k))

        def step():
            Prequest.Startall(req)
            Request.Waitall(req)
        sec = timed(c, flush, step, a.iters, a.warmup)
        ok = bool(torch.equal(r[:n], torch.arange(n, dtype=torch.float64, device="cuda") + ((me - 1) % 4) * 1e7))
        return c.p2p_stats(), c.p2p_pool_stats(), sec, ok
    rows = run(comms, body)
    for c in comms:
        c.Free()
    assert all(x[3] for x in rows), "a neighbour message arrived wrong"
    return [row("neighbours26", mode, rows[0][2], totals(rows), msg_bytes=a.msg_bytes, messages_per_rank=K)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--tile", type=int, default=1024)
    ap.add_argument("--msg-bytes", type=int, default=8192)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    flush = torch.zeros(FLUSH_BYTES // 4, dtype=torch.int32, device="cuda")
    rows = []
    for mode in ("isend", "persistent", "persistent_pool_off"):
        rows += halo(a, mode, flush)
    for mode in ("persistent", "persistent_pool_off"):
        rows += neighbours(a, mode, flush)
    text = "\n".join(json.dumps(r) for r in rows)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
