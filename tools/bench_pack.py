"""Time the fused pack kernel (k_pack: mpjx_pack / mpjx_unpack, layout + byte swap + section header in one pass)
against the unswapped move of the same layout and against the two passes a caller needs without it, in ONE
process, the variants of each shape interleaved repeat by repeat (tools/bench_strided.py's method: other work
shares the host).

  python tools/bench_pack.py [--mib 256] [--iters 10] [--repeats 7] [--rotate 3]

DOUBLE, --mib MiB of payload, one-rank communicator; the section at position 8 of the image, so its payload is
16-byte aligned (the swapping copy's 16-B form needs that). Three layouts on the buffer side:
  contiguous   the basic type
  vector       Vector of 4 KiB blocks at a stride of 8 KiB
  indexed512   the 512-block Indexed type of DESIGN.md §4 "Indexed moves": 4 KiB blocks 8 KiB apart, the last
               block of each item one stride further out, so the type does not normalise to a Vector (LDS search)
Per layout and direction (pack = layout -> image, unpack = image -> layout):
  fused        mpjx_pack / mpjx_unpack
  floor        the same bytes moved WITHOUT a swap by the kernel of that layout: k_moves (mpjx_allgather) for the
               contiguous type, k_strided / k_indexed (mpjx_alltoallv_dt at P = 1) for the others
  two_pass     what a caller does today: the derived-type move into (out of) a contiguous scratch, and the byte
               swap of the scratch into (out of) the image's payload: mpjx_allreduce at P = 1 with
               MPJX_FLAG_SEND_BIG_ENDIAN, which is the library's swapping copy (launch_bswap); two launches. For
               the contiguous type the move is dropped: the swapping copy alone. The header write from the host
               that the composition also needs is not timed.
--rotate R cycles every variant over R buffer sets (cold operands). Times are HIP events on the call's stream.
Before timing, the fused image is compared with the two-pass one at the size timed, and the fused unpack with
the source. One JSON line per variant: every repeat's us, min, median, max; then a summary line of ratios of
medians with each variant's spread (max - min).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from mpjexpress_amd import _lib, mpi  # noqa: E402
from mpjexpress_amd.mpi import MPI, Datatype  # noqa: E402

DOUBLE, SUM = 8, 3
SEND_BIG_ENDIAN = 0x4
BLOCK = 4096 // 8  # doubles per block
TABLE = 512
PAY = 16  # the section starts at position 8: its payload is 16-byte aligned, which the swapping copy needs for its 16-B form


def report(name, us, **kw):
    r = dict(case=name, us=[round(x, 2) for x in us], min=round(min(us), 2), median=round(statistics.median(us), 2),
             max=round(max(us), 2), **kw)
    print(json.dumps(r), flush=True)
    return r


def i64(x):
    return (ctypes.c_int64 * 1)(x)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rotate", type=int, default=3)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.lib()
    comm = mpi.smp_world(1, [0])[0]
    h = comm.handle
    st = torch.cuda.Stream()
    sp = ctypes.c_void_p(st.cuda_stream)
    nbytes = a.mib << 20
    n = nbytes // 8
    R = max(1, a.rotate)
    items = n // (TABLE * BLOCK)
    assert items >= 1 and items * TABLE * BLOCK == n, "--mib must be a multiple of 2 MiB"
    vec = Datatype.Vector(TABLE, BLOCK, 2 * BLOCK, MPI.DOUBLE)
    idx = Datatype.Indexed([BLOCK] * TABLE, [2 * BLOCK * i for i in range(TABLE - 1)] + [2 * BLOCK * TABLE], MPI.DOUBLE)
    assert idx.Size() == vec.Size() == TABLE * BLOCK
    # (type code, items, elements the layout spans)
    layouts = {"contiguous": (DOUBLE, n, n), "vector": (vec.code, items, items * vec.Extent()),
               "indexed512": (idx.code, items, items * idx.Extent() + 2 * BLOCK)}
    image = [torch.empty(nbytes + 32, dtype=torch.uint8, device="cuda") for _ in range(R)]
    other = [torch.empty(nbytes + 32, dtype=torch.uint8, device="cuda") for _ in range(R)]  # the two-pass image
    scratch = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(R)]
    status = torch.zeros(1, dtype=torch.int32, device="cuda")

    def chk(rc, what):
        _lib.check(rc, what)

    for lname, (code, count, span) in layouts.items():
        wide = [torch.randint(-(1 << 62), 1 << 62, (span,), dtype=torch.int64, device="cuda") for _ in range(R)]
        back = [torch.zeros(span, dtype=torch.int64, device="cuda") for _ in range(R)]

        def move(src, sc, stype, dst, rc, rtype):
            if stype == DOUBLE and rtype == DOUBLE:
                chk(L.mpjx_allgather(h, src, dst, sc, DOUBLE, sp), "mpjx_allgather")
            else:
                chk(L.mpjx_alltoallv_dt(h, src, i64(sc), i64(0), stype, dst, i64(rc), i64(0), rtype, sp), "mpjx_alltoallv_dt")

        def swap_copy(dst, src):  # dst = byte-swapped src, n doubles: the library's swapping copy at P = 1
            chk(L.mpjx_allreduce(h, src, dst, n, DOUBLE, SUM, SEND_BIG_ENDIAN, sp), "mpjx_allreduce")

        def fused_pack(k, img=image):
            pos = ctypes.c_int64(8)
            chk(L.mpjx_pack(h, wide[k].data_ptr(), count, code, img[k].data_ptr(), nbytes + 32, ctypes.byref(pos), sp), "mpjx_pack")

        def fused_unpack(k):
            pos = ctypes.c_int64(8)
            chk(L.mpjx_unpack(h, image[k].data_ptr(), nbytes + 32, ctypes.byref(pos), back[k].data_ptr(), count, code,
                              status.data_ptr(), sp), "mpjx_unpack")

        def floor_pack(k):
            move(wide[k].data_ptr(), count, code, image[k].data_ptr() + PAY, n, DOUBLE)

        def floor_unpack(k):
            move(image[k].data_ptr() + PAY, n, DOUBLE, back[k].data_ptr(), count, code)

        def two_pass_pack(k, img=image):
            if code == DOUBLE:
                return swap_copy(img[k].data_ptr() + PAY, wide[k].data_ptr())
            move(wide[k].data_ptr(), count, code, scratch[k].data_ptr(), n, DOUBLE)
            swap_copy(img[k].data_ptr() + PAY, scratch[k].data_ptr())

        def two_pass_unpack(k):
            if code == DOUBLE:
                return swap_copy(back[k].data_ptr(), image[k].data_ptr() + PAY)
            swap_copy(scratch[k].data_ptr(), image[k].data_ptr() + PAY)
            move(scratch[k].data_ptr(), n, DOUBLE, back[k].data_ptr(), count, code)

        # the fused calls are right at the size timed: the same payload as the two passes, the header, the round trip
        torch.cuda.synchronize()
        fused_pack(0)
        two_pass_pack(0, other)
        torch.cuda.synchronize()
        assert torch.equal(image[0][PAY:PAY + nbytes], other[0][PAY:PAY + nbytes]), f"{lname}: fused and two-pass payloads differ"
        assert image[0][8:16].tolist() == [DOUBLE - 1, 0, 0, 0] + list(n.to_bytes(4, "big")), f"{lname}: header"
        fused_unpack(0)
        torch.cuda.synchronize()
        assert int(status.item()) == 0
        probe = torch.empty(nbytes + 32, dtype=torch.uint8, device="cuda")
        pos = ctypes.c_int64(8)
        chk(L.mpjx_pack(h, back[0].data_ptr(), count, code, probe.data_ptr(), nbytes + 32, ctypes.byref(pos), sp), "mpjx_pack")
        torch.cuda.synchronize()
        assert torch.equal(probe[8:PAY + nbytes], image[0][8:PAY + nbytes]), f"{lname}: the unpacked buffer packs to another image"
        del probe
        for d, variants in (("pack", {"fused": fused_pack, "floor": floor_pack, "two_pass": two_pass_pack}),
                            ("unpack", {"fused": fused_unpack, "floor": floor_unpack, "two_pass": two_pass_unpack})):
            times = timed(a, st, variants, R)
            out = {name: report(f"{lname}_{d}_{name}", us, MiB=a.mib, rotate=R, iters=a.iters,
                                GBps_moved=round(2 * nbytes / statistics.median(us) / 1e3, 1))
                   for name, us in times.items()}
            m = {k: v["median"] for k, v in out.items()}
            print(json.dumps({"case": f"{lname}_{d}_summary", "fused_over_floor": round(m["fused"] / m["floor"], 4),
                              "fused_over_two_pass": round(m["fused"] / m["two_pass"], 4),
                              "spread_us": {k: round(v["max"] - v["min"], 2) for k, v in out.items()}}), flush=True)
        del wide, back
    vec.Free()
    idx.Free()
    comm.Free()


if __name__ == "__main__":
    main()
