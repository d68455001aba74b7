"""Time Allreduce(SUM, DOUBLE) on a derived datatype (mpjx_allreduce_dt, the layout-direct kernel k_pway_dt)
against what a caller runs without it, in ONE process, the variants of each shape interleaved repeat by repeat
(tools/bench_strided.py's method: other work shares the host).

  python tools/bench_reduce_dt.py [--ranks 4,8] [--iters 200] [--repeats 7] [--out profiles/reduce_dt/NAME.jsonl]

P rank threads on one device, 1 MiB packed per rank (the configs[0] shape), per blocking call on rank 0's host
clock (each call followed by mpjx_comm_synchronize, the mirrors' blocking form), --iters calls per repeat:
  (a)  mpjx_allreduce_dt on the type
  (b)  what a caller does without it: torch pack, mpjx_allreduce on the packed buffer, torch unpack
  (c)  the floor: mpjx_allreduce on the same packed bytes, contiguous
Shapes: Vector blocks of 4 KiB at stride 8 KiB, 128 B at 256 B and 8 B at 16 B, and one 512-block Indexed type
(2 KiB blocks at irregular displacements). After every repeat each variant's result is checked against (c)'s
result scattered through the layout. One JSON line per variant: every repeat's us, min, median, max; then a
summary line per shape with (a)/(b), (a)/(c) and whether each pair lies outside both variants' spreads.
The 64 MiB cold rows (HIP events, rotated operands) are not part of this tool yet.
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

DOUBLE, SUM = 8, 3
N = (1 << 20) // 8  # packed doubles per rank
SHAPES = (("vector_4096B_of_8192B", 4096, 8192), ("vector_128B_of_256B", 128, 256), ("vector_8B_of_16B", 8, 16),
          ("indexed_512_blocks", 0, 0))
OUT = []


def report(name, us, **kw):
    r = dict(case=name, us=[round(x, 2) for x in us], min=round(min(us), 2), median=round(statistics.median(us), 2),
             max=round(max(us), 2), **kw)
    print(json.dumps(r), flush=True)
    OUT.append(r)
    return r


def layout(name, bb, sb):
    """(make the library type, packed-order element indices, elements spanned)"""
    if bb:
        nb, bl, st = (N * 8) // bb, bb // 8, sb // 8
        idx = (torch.arange(nb)[:, None] * st + torch.arange(bl)[None, :]).reshape(-1)
        return (lambda: Datatype.Vector(nb, bl, st, MPI.DOUBLE)), idx, (nb - 1) * st + bl
    bl = N // 512
    disp = [i * (bl + bl // 2) + (i % 3) * 8 for i in range(512)]
    idx = (torch.tensor(disp)[:, None] + torch.arange(bl)[None, :]).reshape(-1)
    return (lambda: Datatype.Indexed([bl] * 512, disp, MPI.DOUBLE)), idx, disp[-1] + bl


def world(P, a):
    L = _lib.lib()
    comms = mpi.smp_world(P, [0] * P)
    bar = threading.Barrier(P)
    for name, bb, sb in SHAPES:
        make, idx_cpu, span = layout(name, bb, sb)
        idx = idx_cpu.cuda()
        wide = [torch.randint(-1000, 1000, (span,), device="cuda").double() for _ in range(P)]
        out_a = [torch.full((span,), -7.0, dtype=torch.float64, device="cuda") for _ in range(P)]
        out_b = [torch.full((span,), -7.0, dtype=torch.float64, device="cuda") for _ in range(P)]
        packed = [w[idx].contiguous() for w in wide]
        stage = [torch.empty(N, dtype=torch.float64, device="cuda") for _ in range(P)]
        res_c = [torch.empty(N, dtype=torch.float64, device="cuda") for _ in range(P)]
        res_b = [torch.empty(N, dtype=torch.float64, device="cuda") for _ in range(P)]
        torch.cuda.synchronize()
        times = {"a_allreduce_dt": [], "b_torch_pack_allreduce_unpack": [], "c_allreduce_contiguous": []}
        forms = [0] * P

        def body(r):
            torch.cuda.set_device(0)
            h = comms[r].handle
            dt = make()

            def sync():
                _lib.check(L.mpjx_comm_synchronize(h), "sync")

            def va():
                _lib.check(L.mpjx_allreduce_dt(h, wide[r].data_ptr(), out_a[r].data_ptr(), 1, dt.code, SUM, 0, None), "a")
                sync()

            def vb():
                if bb:
                    nb, bl, st = (N * 8) // bb, bb // 8, sb // 8
                    stage[r].view(nb, bl).copy_(torch.as_strided(wide[r], (nb, bl), (st, 1)))
                else:
                    torch.index_select(wide[r], 0, idx, out=stage[r])
                torch.cuda.current_stream().synchronize()  # the mirrors synchronise the device before a call
                _lib.check(L.mpjx_allreduce(h, stage[r].data_ptr(), res_b[r].data_ptr(), N, DOUBLE, SUM, 0, None), "b")
                sync()
                if bb:
                    torch.as_strided(out_b[r], (nb, bl), (st, 1)).copy_(res_b[r].view(nb, bl))
                else:
                    out_b[r].index_copy_(0, idx, res_b[r])
                torch.cuda.current_stream().synchronize()

            def vc():
                _lib.check(L.mpjx_allreduce(h, packed[r].data_ptr(), res_c[r].data_ptr(), N, DOUBLE, SUM, 0, None), "c")
                sync()
            calls = {"a_allreduce_dt": va, "b_torch_pack_allreduce_unpack": vb, "c_allreduce_contiguous": vc}
            for rep in range(a.repeats + 1):  # repeat 0 warms every variant
                for vname, call in calls.items():
                    bar.wait(timeout=120)
                    t0 = time.perf_counter()
                    for _ in range(a.iters):
                        call()
                    us = (time.perf_counter() - t0) / a.iters * 1e6
                    if r == 0 and rep > 0:
                        times[vname].append(us)
                torch.cuda.synchronize()
                want = torch.full((span,), -7.0, dtype=torch.float64, device="cuda")
                want[idx] = res_c[r]  # (c)'s result scattered through the layout
                assert torch.equal(out_a[r], want), (name, "a", r)
                assert torch.equal(out_b[r], want), (name, "b", r)
                out_a[r].fill_(-7.0)
                out_b[r].fill_(-7.0)
                torch.cuda.synchronize()
            f = ctypes.c_int(0)
            va()
            _lib.check(L.mpjx_comm_last_dt_form(h, ctypes.byref(f)), "form")
            forms[r] = f.value
            dt.Free()
        th = [threading.Thread(target=body, args=(r,)) for r in range(P)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert all(f == 3 for f in forms), ("not the layout-direct form", forms)
        rows = {v: report(f"P{P}_{name}_{v}", us, P=P, packed_MiB=1, iters=a.iters, shape=name) for v, us in times.items()}

        def apart(x, y):  # the two variants' [min, max] ranges do not meet
            return rows[x]["min"] > rows[y]["max"] or rows[y]["min"] > rows[x]["max"]
        A, B, C = "a_allreduce_dt", "b_torch_pack_allreduce_unpack", "c_allreduce_contiguous"
        s = {"case": f"P{P}_{name}_summary", "a_over_b": round(rows[A]["median"] / rows[B]["median"], 4),
             "a_over_c": round(rows[A]["median"] / rows[C]["median"], 4), "a_b_outside_spreads": apart(A, B),
             "a_c_outside_spreads": apart(A, C)}
        print(json.dumps(s), flush=True)
        OUT.append(s)
    for c in comms:
        c.Free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ranks", default="4,8")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    for P in [int(p) for p in a.ranks.split(",")]:
        world(P, a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in OUT:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
