"""GPU: every cell of the point-to-point move kernels' per-lane code (csrc/mpjx_k_msgs_tile.hpp) through k_msgs and
k_msgs_pool, with two rank threads on device 0.

tests/msgs_cases.py holds the cases: the 16 shifts of the bytes kind (every arm of shift16's dword select and byte
alignment) at the lengths around a vector and a tile, all 256 alignment pairs at one length, and the five granules
of the granule kind for every pair of regular and irregular sides at the counts around a tile, each at the default
tile and at the streaming tile. tests/test_msgs_cases.py proves on the CPU, against the planner, that the cases
cover all 32 + 40 cells. Here rank 1 sends and rank 0 receives and moves: the order of starts and waits is
test_gpu_preq.ordered's, so rank 0 claims the whole batch and the launch counts are exact. Send buffers are seeded
random bytes and must come back unchanged; every receive buffer starts as the 0xA5 sentinel and is compared whole,
gaps and surround included, with what numpy indexing of the two layouts gives. Nothing has a tolerance.

A case cannot quietly run another arm: before a batch starts, with the REAL device pointers of both ranks in hand,
the shift (bytes kind) or the granule (by the rule restated in pack_cases.granule_log) is recomputed and must
equal the case's claim, and the torch allocations must be 16-byte aligned as the case table assumes.

The streaming form has no knob: a launch takes it when its batch carries kStridedStreamBytes (64 MiB) of payload. A
streaming batch therefore carries one 64 MiB ballast message, filled and checked on the device, beside at most 23
cases, and the launch count shows that ballast and cases went out in one launch. That the launch took the 512-lane
non-temporal form is launch_msgs' rule applied to that payload; it is not observed.

No test provokes a fault: every address a case touches lies inside the tensors allocated here (the census checks
the layouts' spans against the allocation sizes).
"""
import numpy as np
import pytest

import indexed_cases as IC
import msgs_cases as MC
import test_gpu_p2p_halo as H
from mpjexpress_amd.mpi import MPI, Prequest, Request
from test_gpu_preq import dev, free, host, ordered, world

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BALLAST = MC.STREAM_BYTES // 8  # LONGs


@pytest.fixture(scope="module")
def two():
    comms = world(2)
    yield comms
    free(comms)


@pytest.fixture(scope="module")
def ballast():
    """The 64 MiB send and receive buffers of the ballast message, allocated once."""
    torch.cuda.set_device(0)
    s = torch.empty(BALLAST, dtype=torch.int64, device="cuda")
    r = torch.empty(BALLAST, dtype=torch.int64, device="cuda")
    assert s.data_ptr() % 16 == 0 and r.data_ptr() % 16 == 0 and s.numel() * 8 >= MC.STREAM_BYTES
    yield s, r
    del s, r


def ballast_values(out, salt):
    torch.arange(BALLAST, dtype=torch.int64, device="cuda", out=out)
    return out.mul_(2 * salt + 3).add_(salt)


def claim_errors(cases, sptr, rptr):
    """What the real pointers say against the cases' claims."""
    bad = []
    for x, sp, rp in zip(cases, sptr, rptr):
        if sp % 16 or rp % 16:
            bad.append(f"{x.id}: a torch allocation is not 16-byte aligned")
        elif x.kind == "bytes" and x.shift(sp, rp)[0] != x.claim[1]:
            bad.append(f"{x.id}: the pointers give shift {x.shift(sp, rp)[0]}, the case claims {x.claim[1]}")
        elif x.kind == "granule" and x.granule(sp, rp) != x.claim[1]:
            bad.append(f"{x.id}: the pointers give granule {1 << x.granule(sp, rp)} B, the case claims {1 << x.claim[1]} B")
    return bad


def exchange(comms, batches, mode="isend", ballast=None):
    """Every batch of cases from rank 1 to rank 0; what differs, named by the case. mode: "isend" (Isend / Irecv /
    Waitall, one table launch per 24 segments asserted), "send" (blocking Send / Recv, case by case: every one through the
    eager slab, asserted) or "persistent" (Send_init / Recv_init, started twice: the table path and the puts, then ONE k_msgs_pool
    launch, both asserted). With `ballast` every batch carries the 64 MiB message as its last segment."""
    ptrs = {}

    def body(c):
        me, bad, types = c.Rank(), [], {}

        def arg(side):
            if side.contiguous:
                return MPI.BYTE, side.items
            if side.spec not in types:
                types[side.spec] = IC.lib_type(side.f)
            return types[side.spec], side.items

        def post(k, side, buf, send, recv):
            dt, n = arg(side)
            return send(buf, side.off, n, dt, 0, k) if me == 1 else recv(buf, side.off, n, dt, 1, k)

        def verify(cases, bufs, srcs, salt, what):
            for x, buf, src in zip(cases, bufs, srcs):
                exp = src if me == 1 else x.expected(src)
                m = differs(host(buf), exp, f"{x.id} {what}" + (" (send buffer)" if me == 1 else ""))
                if m:
                    bad.append(m)
            if ballast is not None and me == 0:
                exp = ballast_values(torch.empty_like(ballast[1]), salt)
                if not torch.equal(ballast[1], exp):
                    bad.append(f"ballast {what}: {int((ballast[1] != exp).sum())} of {BALLAST} LONGs differ")
                del exp

        try:
            for b, cases in enumerate(batches):
                sides = [x.send if me == 1 else x.recv for x in cases]
                nseg = len(cases) + (ballast is not None)
                tables = -(-nseg // MC.MSGS_MAX)
                bufs = [torch.empty(s.alloc(), dtype=torch.uint8, device="cuda") for s in sides]
                ptrs[me] = [t.data_ptr() for t in bufs]
                c.Barrier()
                if me == 0:
                    bad += claim_errors(cases, ptrs[1], ptrs[0])
                req = []
                if mode == "persistent":
                    req = [post(k, s, t, c.Send_init, c.Recv_init) for k, (s, t) in enumerate(zip(sides, bufs))]
                    if ballast is not None:
                        req.append(c.Send_init(ballast[0], 0, BALLAST, MPI.LONG, 0, len(cases)) if me == 1 else
                                   c.Recv_init(ballast[1], 0, BALLAST, MPI.LONG, 1, len(cases)))
                for it in range(2 if mode == "persistent" else 1):
                    salt = 1000 * b + 100 * it
                    srcs = [x.source(salt + k) for k, x in enumerate(cases)]
                    for t, src in zip(bufs, srcs):
                        if me == 1:
                            t.copy_(dev(src))
                        else:
                            t.fill_(MC.SENT)
                    if ballast is not None and me == 1:
                        ballast_values(ballast[0], salt)
                    elif ballast is not None:
                        ballast[1].fill_(-1)
                    what = f"batch {b} iteration {it} ({mode})"
                    if mode == "send":
                        eager = c.p2p_stats()[2]
                        for k, (s, t) in enumerate(zip(sides, bufs)):
                            post(k, s, t, c.Send, c.Recv)
                        c.Barrier()
                        if me == 1 and c.p2p_stats()[2] - eager != len(cases):
                            bad.append(f"{what}: {c.p2p_stats()[2] - eager} of {len(cases)} sends were eager")
                        verify(cases, bufs, srcs, salt, what)
                        continue

                    def start():
                        if mode == "persistent":
                            return Prequest.Startall(req)
                        req[:] = [post(k, s, t, c.Isend, c.Irecv) for k, (s, t) in enumerate(zip(sides, bufs))]
                        if ballast is not None:
                            req.append(c.Isend(ballast[0], 0, BALLAST, MPI.LONG, 0, len(cases)) if me == 1 else
                                       c.Irecv(ballast[1], 0, BALLAST, MPI.LONG, 1, len(cases)))
                    before = (c.p2p_stats()[0],) + c.p2p_pool_stats()[:3]
                    ordered(c, 0, start, lambda: Request.Waitall(req))
                    after = (c.p2p_stats()[0],) + c.p2p_pool_stats()[:3]
                    delta = tuple(x - y for x, y in zip(after, before))
                    if me == 1:
                        want = (0, 0, 0, 0)
                    elif mode == "persistent":  # (launches, pool launches, puts, hits)
                        want = ((tables, 0, nseg, 0), (1, 1, 0, nseg))[it]
                    else:
                        want = (tables, 0, 0, 0)
                    if delta != want:
                        bad.append(f"{what}: rank {me} counted (launches, pool launches, puts, hits) = {delta}, planned {want}")
                    verify(cases, bufs, srcs, salt, what)
                if mode == "persistent":  # Waitall has freed the plain requests
                    for q in req:
                        q.Free()
                c.Barrier()
        finally:
            for t in types.values():
                t.Free()
        return bad

    out = H.run_ranks(comms, body, limit=120)
    return out[0] + out[1]


def differs(got, exp, what):
    if np.array_equal(got, exp):
        return None
    wrong = np.flatnonzero(got != exp)
    return (f"{what}: {wrong.size} of {exp.size} bytes differ, the first at byte {wrong[0]} "
            f"(got {got[wrong[0]]:#x}, expected {exp[wrong[0]]:#x})")


def batches_of(cases, n=MC.MSGS_MAX):
    return [cases[i:i + n] for i in range(0, len(cases), n)]


SHIFTS = pytest.mark.parametrize("sh", range(16), ids=lambda s: f"sh{s}")
GRANULES = pytest.mark.parametrize("glog", range(5), ids=lambda g: f"g{g}")


# ---- the default tile ---------------------------------------------------------------------------------------------

@SHIFTS
def test_bytes_shift(two, sh):
    """One arm of shift16 (q = sh >> 2, b = sh & 3) in k_msgs<false>: 5 B across a 16-byte line, and one vector, one
    tile, one tile and a vector and two tiles less a byte at an aligned destination and at one with head and tail."""
    bad = exchange(two, [MC.bytes_cases(sh, "default")])
    assert not bad, "\n".join(bad)


@SHIFTS
def test_bytes_shift_through_blocking_send(two, sh):
    """The same messages through Send: the eager slab, so each one is moved twice, at the slab's alignment between."""
    bad = exchange(two, [MC.bytes_cases(sh, "default")], mode="send")
    assert not bad, "\n".join(bad)


def test_alignment_sweep(two):
    """All 16 x 16 (src & 15, dst & 15) at 4099 B, 24 messages to a launch."""
    bad = exchange(two, batches_of(MC.sweep_cases()))
    assert not bad, "\n".join(bad)


@GRANULES
def test_granule(two, glog):
    """granule_tile<false, glog> with regular and irregular sides in all four pairings, at 1, 1023, 1024, 1025 and
    2049 granules, and the message that ends inside the last receive item on a tile's edge."""
    bad = exchange(two, [MC.granule_cases(glog, "default")])
    assert not bad, "\n".join(bad)


def test_full_table_takes_two_launches(two):
    """25 segments of both kinds in turn, of one tile and of three: kMsgsMax = 24 in the first launch, one in the
    second (the launch count is asserted in exchange)."""
    cases = MC.full_table()
    assert len(cases) == MC.MSGS_MAX + 1
    bad = exchange(two, [cases])
    assert not bad, "\n".join(bad)


# ---- the streaming tile ----------------------------------------------------------------------------------------------

@SHIFTS
def test_bytes_shift_streaming(two, ballast, sh):
    """The arm in k_msgs<true>: the same lengths around the 512-vector tile, beside the ballast, in ONE launch."""
    bad = exchange(two, [MC.bytes_cases(sh, "nt")], ballast=ballast)
    assert not bad, "\n".join(bad)


@GRANULES
def test_granule_streaming(two, ballast, glog):
    """granule_tile<true, glog>: 1, 511, 512, 513 and 1025 granules, beside the ballast, in ONE launch."""
    bad = exchange(two, [MC.granule_cases(glog, "nt")], ballast=ballast)
    assert not bad, "\n".join(bad)


# ---- the pool --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tile", MC.TILES)
def test_pool(ballast, tile):
    """Persistent requests: the 16 shifts and the irregular-to-irregular row of the five granules, started twice. The
    first start takes the table path and stores every segment; the second is one k_msgs_pool launch, of
    k_msgs_pool<true> where the persistent ballast is among the pairs."""
    comms = world(2)
    try:
        bad = exchange(comms, [MC.pool_cases(tile)], mode="persistent", ballast=ballast if tile == "nt" else None)
    finally:
        free(comms)
    assert not bad, "\n".join(bad)
