"""Wire-format message timing: a typed -> MPI.PACKED message and a MPI.PACKED -> typed message (k_wire: layout, byte
swap and header in one pass) between two rank threads, against

  pack_alone / unpack_alone   (a) mpjx_pack / mpjx_unpack alone on the same layout, on the receiving rank: the
                              one-pass floor (k_pack does the same per-lane work, without a message)
  three_pass                  (b) what a caller without MPI.PACKED messages does: mpjx_pack into a scratch image on the
                              sender, Send / Recv of the image as BYTE, mpjx_unpack on the receiver: three passes

  python tools/bench_wire.py [--reps 9] [--warmup 2] [--sizes 268435456,65536,8192] [--out FILE]

The layout is DOUBLE as a Vector of 4 KiB blocks, 8 KiB apart; --sizes are payload bytes. The variants are
interleaved repeat by repeat in one process. Times are host wall-clock on the RECEIVING rank, from the barrier
before the exchange to its blocking call's return, on cold operands: before every timed run rank 0 rewrites a
512 MiB scratch buffer, twice the 256 MiB Infinity Cache the ranks share, outside the timed region. One JSON line per
(size, variant): the median with the minimum and the maximum."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from mpjexpress_amd import mpi  # noqa: E402
from mpjexpress_amd.mpi import MPI, Datatype  # noqa: E402

FLUSH_BYTES = 512 << 20
BLOCK = 512  # doubles per block: 4 KiB
VARIANTS = ("wire_pack", "wire_unpack", "pack_alone", "unpack_alone", "three_pass")


def run(comms, fn):
    out, err = [None] * len(comms), [None] * len(comms)

    def body(r):
        try:
            torch.cuda.set_device(0)
            out[r] = fn(comms[r])
        except BaseException as e:  # noqa: BLE001
            err[r] = e
    ts = [threading.Thread(target=body, args=(r,)) for r in range(len(comms))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for e in err:
        if e is not None:
            raise e
    return out


def bench(size, reps, warmup):
    nblk = size // (BLOCK * 8)
    assert nblk >= 1 and nblk * BLOCK * 8 == size, "sizes are whole 4 KiB blocks"
    comms = mpi.smp_world(2, [0, 0])
    vec = Datatype.Vector(nblk, BLOCK, 2 * BLOCK, MPI.DOUBLE)
    room = 8 + size

    def body(c):
        me = c.Rank()
        c.set_p2p_timeout(120)
        buf = torch.arange(2 * BLOCK * nblk, dtype=torch.float64, device="cuda") + me  # the typed side
        img = torch.zeros(room, dtype=torch.uint8, device="cuda")                      # the image side
        flush = torch.zeros(FLUSH_BYTES // 4, dtype=torch.int32, device="cuda") if me == 0 else None
        c.Pack(buf, 0, 1, vec, img, 0)  # a valid section on both ranks

        def step(v):
            if v == "wire_pack":
                if me == 0:
                    c.Isend(buf, 0, 1, vec, 1, 1).Wait()
                else:
                    c.Recv(img, 0, room, MPI.PACKED, 0, 1)
            elif v == "wire_unpack":
                if me == 0:
                    c.Isend(img, 0, room, MPI.PACKED, 1, 2).Wait()
                else:
                    c.Recv(buf, 0, 1, vec, 0, 2)
            elif v == "pack_alone":
                if me == 1:
                    c.Pack(buf, 0, 1, vec, img, 0)
            elif v == "unpack_alone":
                if me == 1:
                    c.Unpack(img, 0, buf, 0, 1, vec)
            else:
                if me == 0:
                    c.Pack(buf, 0, 1, vec, img, 0)
                    c.Isend(img, 0, room, MPI.BYTE, 1, 3).Wait()
                else:
                    c.Recv(img, 0, room, MPI.BYTE, 0, 3)
                    c.Unpack(img, 0, buf, 0, 1, vec)

        ts = {v: [] for v in VARIANTS}
        for i in range(warmup + reps):
            for v in VARIANTS:  # interleaved: every repeat runs every variant
                if me == 0:
                    flush.add_(1)  # evicts the shared cache; rank 1 waits at the barrier
                    torch.cuda.synchronize()
                c.Barrier()
                t0 = time.perf_counter()
                step(v)
                t1 = time.perf_counter()
                c.Barrier()
                if i >= warmup:
                    ts[v].append(t1 - t0)
        return ts
    out = run(comms, body)[1]  # the receiving rank's clock
    for c in comms:
        c.Free()
    vec.Free()
    rows = []
    for v in VARIANTS:
        us = [t * 1e6 for t in out[v]]
        med = statistics.median(us)
        rows.append({"bench": "wire", "payload_bytes": size, "layout": f"Vector({nblk}, {BLOCK}, {2 * BLOCK}, DOUBLE)",
                     "variant": v, "median_us": round(med, 2), "min_us": round(min(us), 2), "max_us": round(max(us), 2),
                     "payload_GBps_at_median": round(size / med / 1e3, 2), "reps": len(us)})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="268435456,65536,8192")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rows = []
    for size in [int(s) for s in a.sizes.split(",")]:
        rows += bench(size, a.reps, a.warmup)
    text = "".join(json.dumps(r) + "\n" for r in rows)
    sys.stdout.write(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
