"""Time the indexed block-move kernel (k_indexed: mpjx_alltoallv_dt with an Indexed type on one side) against
what it is built on and what it replaces, in ONE process, the variants of each shape interleaved repeat by
repeat (tools/bench_strided.py's method: other work shares the host).

  python tools/bench_indexed.py [--mib 256] [--iters 10] [--repeats 7] [--rotate 3] [--table 4096]
                                [--forms] [--t-iters 200] [--skip-floor] [--skip-perm] [--skip-world]

DOUBLE, --mib MiB packed, P = 1; block bytes 8, 128 and 4096. A type holds --table blocks; the message is as
many items of it as fill --mib.
floor     blocks 2 x their length apart, the last block of each item one stride further out, so the type does
          not normalise to a Vector. Gather (Indexed -> contiguous) and scatter against k_strided on the Vector
          of the same blocks and against k_moves on the same number of contiguous bytes.
perm      a random permutation of the item's blocks (dense: the item is its blocks, shuffled). Gather and
          scatter against torch moving the same bytes with an index tensor already on the device: by element
          (dst.copy_(src[idx]), index_copy_) and by row of a (blocks, block length) view (index_select with
          out=, index_copy_), whichever is faster.
--forms   adds k_indexed with the search forced to its direct form and to its LDS form (tables of up to 512
          blocks; MPJX_INDEXED_LDS_MAX_BLOCKS, read per call) beside the default, on the same bytes.
world     P = 4 rank threads on one device: Alltoallv with an Indexed send type (256 ragged rows, 1 MiB per
          rank pair) against torch's pack of the same rows followed by mpjx_alltoallv, each followed by
          mpjx_comm_synchronize (the mirrors' blocking form); host clock of rank 0 per call.
--rotate R cycles every variant over R buffer sets (cold operands). Times are HIP events on the call's stream.
One JSON line per variant: every repeat's us, min, median, max; then a summary line of ratios of medians with
each variant's spread (max - min).
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
BLOCKS = (8, 128, 4096)


def report(name, us, **kw):
    r = dict(case=name, us=[round(x, 2) for x in us], min=round(min(us), 2), median=round(statistics.median(us), 2),
             max=round(max(us), 2), **kw)
    print(json.dumps(r), flush=True)
    return r


def i64(x):
    return (ctypes.c_int64 * 1)(x)


def lds(fn, blocks):
    def go(k):
        os.environ["MPJX_INDEXED_LDS_MAX_BLOCKS"] = str(blocks)
        try:
            fn(k)
        finally:
            del os.environ["MPJX_INDEXED_LDS_MAX_BLOCKS"]
    return go


def timed(a, st, variants, R):
    for go in variants.values():  # warm every variant on every buffer set
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
    return times


def summary(case, out, pairs):
    m = {k: v["median"] for k, v in out.items()}
    s = {"case": case}
    for name, (x, y) in pairs.items():
        if x in m and y in m:
            s[name] = round(m[x] / m[y], 4)
    s["spread_us"] = {k: round(v["max"] - v["min"], 2) for k, v in out.items()}
    print(json.dumps(s), flush=True)


def one_rank(a):
    L = _lib.lib()
    comm = mpi.smp_world(1, [0])[0]
    h = comm.handle
    st = torch.cuda.Stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    nbytes = a.mib << 20
    n = nbytes // 8
    R = max(1, a.rotate)
    T = a.table
    packed = [torch.randint(0, 1 << 40, (n,), dtype=torch.int64, device="cuda") for _ in range(R)]
    flat = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(R)]

    def dt(src, sc, stype, dst, rc, rtype):
        _lib.check(L.mpjx_alltoallv_dt(h, src.data_ptr(), i64(sc), i64(0), stype, dst.data_ptr(), i64(rc), i64(0), rtype, sp),
                   "mpjx_alltoallv_dt")

    for bb in BLOCKS:
        bl = bb // 8
        items = nbytes // (T * bb)
        assert items >= 1 and items * T * bb == nbytes, "--mib must be a multiple of table x block bytes"
        if not a.skip_floor:
            stl = 2 * bl
            vec = Datatype.Vector(T, bl, stl, MPI.DOUBLE)
            idx = Datatype.Indexed([bl] * T, [stl * i for i in range(T - 1)] + [stl * T], MPI.DOUBLE)
            assert idx.Size() == vec.Size() == T * bl and idx.Extent() == vec.Extent() + stl
            wide = [torch.randint(0, 1 << 40, (items * idx.Extent() + stl,), dtype=torch.int64, device="cuda") for _ in range(R)]
            variants = {
                "gather_indexed": lambda k: dt(wide[k], items, idx.code, flat[k], n, DOUBLE),
                "scatter_indexed": lambda k: dt(packed[k], n, DOUBLE, wide[k], items, idx.code),
                "gather_vector": lambda k: dt(wide[k], items, vec.code, flat[k], n, DOUBLE),
                "scatter_vector": lambda k: dt(packed[k], n, DOUBLE, wide[k], items, vec.code),
                "k_moves_contiguous": lambda k: _lib.check(L.mpjx_allgather(h, packed[k].data_ptr(), flat[k].data_ptr(), n, DOUBLE, sp),
                                                           "mpjx_allgather"),
            }
            if a.forms and T <= 512:
                for d in ("gather", "scatter"):
                    variants[f"{d}_indexed_direct"] = lds(variants[f"{d}_indexed"], 0)
                    variants[f"{d}_indexed_lds"] = lds(variants[f"{d}_indexed"], 512)
            # the moves are right at the size timed: item k's block b, and the displaced last block
            torch.cuda.synchronize()  # the operands were made on another stream
            variants["gather_indexed"](0)
            torch.cuda.synchronize()
            w = wide[0][:items * idx.Extent()].view(items, idx.Extent())
            got = flat[0].view(items, T, bl)
            assert torch.equal(got[:, :T - 1], w[:, :(T - 1) * stl].reshape(items, T - 1, stl)[:, :, :bl]), "gather differs"
            assert torch.equal(got[:, T - 1], w[:, T * stl:T * stl + bl]), "gather differs in the displaced block"
            times = timed(a, st, variants, R)
            out = {name: report(f"floor_{bb}B_{name}", us, MiB=a.mib, rotate=R, iters=a.iters, block_bytes=bb, table_blocks=T,
                                items=items, GBps_moved=round(2 * nbytes / statistics.median(us) / 1e3, 1))
                   for name, us in times.items()}
            summary(f"floor_{bb}B_summary", out, {
                "gather_indexed_over_vector": ("gather_indexed", "gather_vector"),
                "scatter_indexed_over_vector": ("scatter_indexed", "scatter_vector"),
                "gather_indexed_over_k_moves": ("gather_indexed", "k_moves_contiguous"),
                "scatter_indexed_over_k_moves": ("scatter_indexed", "k_moves_contiguous"),
                "gather_lds_over_direct": ("gather_indexed_lds", "gather_indexed_direct"),
                "scatter_lds_over_direct": ("scatter_indexed_lds", "scatter_indexed_direct")})
            vec.Free()
            idx.Free()
            del wide, variants
        if not a.skip_perm:
            g = torch.Generator().manual_seed(bb)
            order = torch.randperm(T, generator=g)
            perm = Datatype.Indexed([bl] * T, [int(i) * bl for i in order], MPI.DOUBLE)  # dense: extent = size
            assert perm.Size() == perm.Extent() == T * bl
            rows = (torch.arange(items)[:, None] * T + order[None, :]).reshape(-1).cuda()  # packed row -> source row
            elem = (rows[:, None] * bl + torch.arange(bl, device="cuda")[None, :]).reshape(-1)
            src2 = [p.view(-1, bl) for p in packed]
            dst2 = [f.view(-1, bl) for f in flat]

            def on(fn):
                def go(k):
                    with torch.cuda.stream(st):
                        fn(k)
                return go
            variants = {
                "gather_indexed": lambda k: dt(packed[k], items, perm.code, flat[k], n, DOUBLE),
                "scatter_indexed": lambda k: dt(packed[k], n, DOUBLE, flat[k], items, perm.code),
                "torch_gather_elements": on(lambda k: flat[k].copy_(packed[k][elem])),
                "torch_gather_rows": on(lambda k: torch.index_select(src2[k], 0, rows, out=dst2[k])),
                "torch_scatter_elements": on(lambda k: flat[k].index_copy_(0, elem, packed[k])),
                "torch_scatter_rows": on(lambda k: dst2[k].index_copy_(0, rows, src2[k])),
            }
            if a.forms and T <= 512:
                for d in ("gather", "scatter"):
                    variants[f"{d}_indexed_direct"] = lds(variants[f"{d}_indexed"], 0)
                    variants[f"{d}_indexed_lds"] = lds(variants[f"{d}_indexed"], 512)
            torch.cuda.synchronize()  # the operands were made on another stream
            variants["gather_indexed"](0)
            torch.cuda.synchronize()
            assert torch.equal(flat[0], packed[0][elem]), "gather differs"
            variants["scatter_indexed"](0)
            torch.cuda.synchronize()
            assert torch.equal(flat[0][elem], packed[0]), "scatter differs"
            times = timed(a, st, variants, R)
            out = {name: report(f"perm_{bb}B_{name}", us, MiB=a.mib, rotate=R, iters=a.iters, block_bytes=bb, table_blocks=T,
                                items=items, GBps_moved=round(2 * nbytes / statistics.median(us) / 1e3, 1))
                   for name, us in times.items()}
            m = {k: v["median"] for k, v in out.items()}
            tg = min(("torch_gather_elements", "torch_gather_rows"), key=lambda k: m[k])
            ts = min(("torch_scatter_elements", "torch_scatter_rows"), key=lambda k: m[k])
            summary(f"perm_{bb}B_summary", out, {
                f"gather_indexed_over_{tg}": ("gather_indexed", tg),
                f"scatter_indexed_over_{ts}": ("scatter_indexed", ts),
                "gather_lds_over_direct": ("gather_indexed_lds", "gather_indexed_direct"),
                "scatter_lds_over_direct": ("scatter_indexed_lds", "scatter_indexed_direct")})
            perm.Free()
            del rows, elem, variants
    comm.Free()


def world(a, P=4):
    L = _lib.lib()
    comms = mpi.smp_world(P, [0] * P)
    nrows, bw = 256, 1024  # a block: 256 ragged rows out of 1024 columns; 512 doubles a row on average = 1 MiB
    N = P * bw
    lens = [512 + 128 * (i % 3 - 1) for i in range(nrows - 1)]
    lens.append(nrows * 512 - sum(lens))
    blk = sum(lens)
    panel = [torch.randint(0, 1 << 40, (nrows * N,), dtype=torch.int64, device="cuda") for _ in range(P)]
    pack = [torch.empty(P * blk, dtype=torch.int64, device="cuda") for _ in range(P)]
    recv = [torch.empty(P * blk, dtype=torch.int64, device="cuda") for _ in range(P)]
    one = torch.cat([i * N + torch.arange(n) for i, n in enumerate(lens)])
    elem = torch.cat([one + bw * j for j in range(P)]).cuda()  # the element index of the whole pack
    torch.cuda.synchronize()
    times = {"alltoallv_indexed": [], "torch_pack_then_alltoallv": []}
    bar = threading.Barrier(P)
    arr = ctypes.c_int64 * P

    def body(r):
        torch.cuda.set_device(0)
        h = comms[r].handle
        block = Datatype.Indexed(lens, [i * N for i in range(nrows)], MPI.DOUBLE)
        sc, sd = arr(*[1] * P), arr(*[bw * j for j in range(P)])
        pc, pd = arr(*[blk] * P), arr(*[blk * i for i in range(P)])

        def indexed():
            _lib.check(L.mpjx_alltoallv_dt(h, panel[r].data_ptr(), sc, sd, block.code, recv[r].data_ptr(), pc, pd, DOUBLE,
                                           None), "mpjx_alltoallv_dt")
            _lib.check(L.mpjx_comm_synchronize(h), "sync")

        def packed():
            torch.index_select(panel[r], 0, elem, out=pack[r])
            torch.cuda.current_stream().synchronize()  # the mirrors synchronise the device before a call
            _lib.check(L.mpjx_alltoallv(h, pack[r].data_ptr(), pc, pd, recv[r].data_ptr(), pc, pd, DOUBLE, None), "mpjx_alltoallv")
            _lib.check(L.mpjx_comm_synchronize(h), "sync")
        calls = {"alltoallv_indexed": indexed, "torch_pack_then_alltoallv": packed}
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
                for i in range(P):  # either way: block i of rank r = rank i's ragged rows of column block r
                    assert torch.equal(recv[r][i * blk:(i + 1) * blk], panel[i][elem[r * blk:(r + 1) * blk]]), (name, r, i)
                recv[r].zero_()
                torch.cuda.synchronize()
        block.Free()
    th = [threading.Thread(target=body, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    out = {name: report(f"world_P{P}_{name}", us, P=P, block_MiB=1, iters=a.t_iters) for name, us in times.items()}
    summary(f"world_P{P}_summary", out, {"indexed_over_torch_pack": ("alltoallv_indexed", "torch_pack_then_alltoallv")})
    for c in comms:
        c.Free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rotate", type=int, default=3)
    ap.add_argument("--table", type=int, default=4096)
    ap.add_argument("--t-iters", type=int, default=200)
    ap.add_argument("--forms", action="store_true")
    ap.add_argument("--skip-floor", action="store_true")
    ap.add_argument("--skip-perm", action="store_true")
    ap.add_argument("--skip-world", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if not (a.skip_floor and a.skip_perm):
        one_rank(a)
    if not a.skip_world:
        world(a)


if __name__ == "__main__":
    main()
