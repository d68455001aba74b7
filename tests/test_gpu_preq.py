"""GPU: persistent requests (Send_init, Recv_init, Prequest.Start / Startall) on device buffers, and the device
segment pool behind them (k_msgs_pool), with rank threads in-process on device 0 under a time limit per world.

  - the known answers of the reference's test/mpi/pt2pt/start.java (first phase), startall.java, TestSendInit.java
    and start2.java (its Send_init / Recv_init pair): data[i] == i, Get_count(INT) == 1 on the receive statuses,
    the empty status on sends; the expected values are the programs' own checks
  - reuse, a 2 x 2 halo compared byte for byte with the same exchange through Isend / Irecv, with the pool, with
    MPJX_P2P_POOL=0 and with MPJX_P2P_BATCH=0
  - the launch counts of the pool (30 pairs, above k_msgs' 24 per launch, in ONE launch; 513 in two), tile
    boundaries, the streaming form, subsets, wildcards, short messages, PROC_NULL, count 0, mixed batches, stale
    slots, a full pool, and the errors
Where launch counts are asserted the order of starts and waits is fixed with barriers (the pattern of
test_gpu_p2p_halo.fixed_order): the peers start first, then ONE rank starts and waits, claiming every pair."""
import contextlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import p2p_cases as PC
import test_gpu_p2p_halo as H
from mpjexpress_amd import mpi
from mpjexpress_amd.mpi import MPI, Datatype, MPIException, Prequest, Request

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = H.N
SLOTS, BATCH_MAX, STREAM_BYTES = 1024, 512, 64 << 20  # kPoolSlots, kPoolBatchMax, kStridedStreamBytes
EMPTY = (MPI.PROC_NULL, MPI.ANY_TAG, 0)


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def world(P, timeout=20, **kv):
    with env(**kv):  # the switches are read once, when the world is created
        comms = mpi.smp_world(P, [0] * P)
    for c in comms:
        c.set_p2p_timeout(timeout)
    return comms


def free(comms):
    for c in comms:
        c.Free()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def triple(st, dt=MPI.INT):
    return st.source, st.tag, st.Get_count(dt)


def ordered(c, mover, start, wait):
    """One iteration in a fixed order: every rank but `mover` starts, Barrier, `mover` starts and waits (claiming
    every pair), Barrier, the others wait. Returns what wait() returned."""
    me = c.Rank()
    if me != mover:
        start()
    c.Barrier()
    out = None
    if me == mover:
        start()
        out = wait()
    c.Barrier()
    if me != mover:
        out = wait()
    c.Barrier()
    return out


def pool_hits(c):
    """The pairs communicator c has moved from its pool. Of mpjx_comm_p2p_pool_stats' values the three counters
    are atomic and may be read from another rank's thread, as here, while c's own thread is inside a wait;
    slots_in_use may not, so it is not asked for."""
    import ctypes

    from mpjexpress_amd import _lib
    hits = ctypes.c_int64()
    assert _lib.lib().mpjx_comm_p2p_pool_stats(c.handle, None, None, ctypes.byref(hits), None, None) == 0
    return hits.value


def inactive(reqs):
    return all((not r.Is_null()) and not r.Is_active() for r in reqs)


# ---- 1. the reference's known answers at P = 4 --------------------------------------------------------------------

@pytest.mark.parametrize("program,rounds,startall,barrier", [("start", 1, False, True), ("startall", 2, True, False),
                                                             ("TestSendInit", 3, False, True)])
def test_reference_known_answers(program, rounds, startall, barrier):
    comms = world(4)

    def body(c):
        me, tasks = c.Rank(), c.Size()
        mebuf = dev(np.array([me], np.int32))
        data = torch.zeros(tasks, dtype=torch.int32, device="cuda")
        req = []
        for rnd in range(rounds):
            if program == "startall" or rnd == 0:  # startall.java makes its requests anew for the second round
                for r in req:
                    r.Free()
                req = []
                for i in range(tasks):
                    req.append(c.Send_init(mebuf, 0, 1, MPI.INT, i, 1))
                    req.append(c.Recv_init(data, i, 1, MPI.INT, i, 1))
                assert inactive(req)
            data.fill_(-1)
            if barrier:
                c.Barrier()
            if startall:
                Prequest.Startall(req)
            else:
                for r in req:
                    r.Start()
            assert all(r.Is_active() for r in req)
            stats = Request.Waitall(req)
            assert host(data).tolist() == list(range(tasks)), (program, rnd, host(data).tolist())
            for i in range(tasks):
                assert triple(stats[2 * i + 1]) == (i, 1, 1), (program, rnd, i)
                assert triple(stats[2 * i]) == EMPTY and stats[2 * i].error == 0  # only the receivers have status values
            assert inactive(req)
        c.Barrier()
        for r in req:
            r.Free()
        assert all(r.Is_null() for r in req)
        return True
    assert H.run_ranks(comms, body) == [True] * 4
    free(comms)


def test_reference_start2_send_init_pair():
    """start2.java's first pair: rank 0 Send_init of X = 100 INTs of -1 to rank 1 under tag 1, rank 1 Recv_init; both
    Start. The program's check is data1[i] == -1 on rank 1 (its Ssend / Bsend / Rsend pairs use modes that do
    not exist here). The wait is ours: the program ends without one."""
    comms = world(4)
    X = 100

    def body(c):
        me = c.Rank()
        data1 = torch.full((X,), -1 if me == 0 else 0, dtype=torch.int32, device="cuda")
        req = None
        if me == 0:
            req = c.Send_init(data1, 0, X, MPI.INT, 1, 1)
        elif me == 1:
            req = c.Recv_init(data1, 0, X, MPI.INT, 0, 1)
        st = None
        if req is not None:
            req.Start()
            st = req.Wait()
            assert inactive([req])
            req.Free()
        c.Barrier()
        return host(data1).tolist(), None if st is None else triple(st)
    out = H.run_ranks(comms, body)
    assert out[1] == ([-1] * X, (0, 1, X)) and out[0] == ([-1] * X, EMPTY) and out[2][1] is None
    free(comms)


# ---- 2. reuse --------------------------------------------------------------------------------------------------------

def test_reuse_sees_the_new_bytes_every_iteration():
    comms = world(2)

    def body(c):
        me, other = c.Rank(), 1 - c.Rank()
        s = torch.zeros(1000, dtype=torch.int32, device="cuda")
        r = torch.full((1000,), -1, dtype=torch.int32, device="cuda")
        rs, rr = c.Send_init(s, 3, 900, MPI.INT, other, 4), c.Recv_init(r, 5, 900, MPI.INT, other, 4)
        seen = []
        for it in range(4):
            s.copy_(torch.arange(1000, dtype=torch.int32, device="cuda") * (it + 1) + 100000 * me)
            Prequest.Startall([rr, rs])
            sts = Request.Waitall([rr, rs])
            assert triple(sts[0]) == (other, 4, 900) and triple(sts[1]) == EMPTY
            assert inactive([rr, rs])
            # a wait or a test on an inactive request returns at once with the empty status
            assert triple(rr.Wait()) == EMPTY and triple(rs.Test()) == EMPTY and inactive([rr, rs])
            assert [triple(x) for x in Request.Waitall([rr, rs])] == [EMPTY, EMPTY]
            exp = np.full(1000, -1, np.int32)
            exp[5:905] = np.arange(3, 903, dtype=np.int32) * (it + 1) + 100000 * other
            seen.append(np.array_equal(host(r), exp))
            c.Barrier()
        rs.Free()
        rr.Free()
        return seen, c.p2p_stats()[1]
    out = H.run_ranks(comms, body)
    assert out[0][0] == [True] * 4 and out[1][0] == [True] * 4
    assert out[0][1] + out[1][1] == 8  # 2 pairs x 4 iterations moved, by one rank or the other
    free(comms)


# ---- 3. halo 2 x 2 ----------------------------------------------------------------------------------------------------

ITERS = 4


def halo_requests(c, t, x, col, idx, persistent):
    nb = H.neighbours(c.Rank())
    at = lambda r, k: r * N + k  # noqa: E731
    recv, send = (c.Recv_init, c.Send_init) if persistent else (c.Irecv, c.Isend)
    return [
        recv(t, at(N - 1, 1), N - 2, MPI.DOUBLE, nb["s"], 0),
        recv(t, at(0, 1), N - 2, MPI.DOUBLE, nb["n"], 1),
        recv(t, at(1, N - 1), 1, col, nb["e"], 2),
        recv(t, at(1, 0), 1, col, nb["w"], 3),
        recv(x, 3, 1, idx, nb["w"], 4),
        send(t, at(1, 1), N - 2, MPI.DOUBLE, nb["n"], 0),
        send(t, at(N - 2, 1), N - 2, MPI.DOUBLE, nb["s"], 1),
        send(t, at(1, 1), 1, col, nb["w"], 2),
        send(t, at(1, N - 2), 1, col, nb["e"], 3),
        send(t, at(5, 1), 1, idx, nb["e"], 4),  # an Indexed selection of row 5 into the neighbour's side buffer
    ]


def halo_body(c, col, idx, persistent):
    me = c.Rank()
    t = torch.from_numpy(H.tile_of(me)).cuda().reshape(-1)
    x = torch.full((40,), -7.0, dtype=torch.float64, device="cuda")  # guard elements around the Indexed receive
    interior = t.view(N, N)[1:N - 1, 1:N - 1]
    req = halo_requests(c, t, x, col, idx, True) if persistent else None
    for it in range(ITERS):
        if persistent:
            Prequest.Startall(req)
            sts = Request.Waitall(req)
            assert inactive(req)
        else:
            sts = Request.Waitall(halo_requests(c, t, x, col, idx, False))
        nb = H.neighbours(me)
        assert [s.source for s in sts[:5]] == [nb["s"], nb["n"], nb["e"], nb["w"], nb["w"]]
        assert [s.tag for s in sts[:5]] == [0, 1, 2, 3, 4]
        interior += 0.5 * (me + 1)  # the next iteration sends new bytes
    c.Barrier()
    if persistent:
        for r in req:
            r.Free()
    return host(t).tobytes(), host(x).tobytes()


def halo(persistent, **kv):
    comms = world(4, **kv)
    col = Datatype.Vector(N - 2, 1, N, MPI.DOUBLE)
    idx = Datatype.Indexed([3, 1, 5], [7, 0, 20], MPI.DOUBLE)
    out = H.run_ranks(comms, lambda c: halo_body(c, col, idx, persistent))
    stats = [c.p2p_pool_stats() for c in comms]
    col.Free()
    idx.Free()
    free(comms)
    return out, stats


@pytest.fixture(scope="module")
def halo_reference():
    """The exchange through Isend / Irecv, computed once and shared."""
    out, stats = halo(False)
    assert all(s[:4] == (0, 0, 0, 0) for s in stats)  # plain requests never reach the pool
    # the last iteration's halo against numpy: rank r's top halo row is its northern neighbour's row N - 2
    for r in range(4):
        t = np.frombuffer(out[r][0], np.float64).reshape(N, N)
        x = np.frombuffer(out[r][1], np.float64)
        nb = H.neighbours(r)
        north = H.tile_of(nb["n"])
        north[1:N - 1, 1:N - 1] += 0.5 * (nb["n"] + 1) * (ITERS - 1)
        assert np.array_equal(t[0, 1:N - 1], north[N - 2, 1:N - 1]), r
        west = H.tile_of(nb["w"])
        west[1:N - 1, 1:N - 1] += 0.5 * (nb["w"] + 1) * (ITERS - 1)
        sel = PC.blocks([3, 1, 5], [7, 0, 20])
        exp = np.full(40, -7.0)
        exp[3 + sel] = west.reshape(-1)[5 * N + 1 + sel]
        assert np.array_equal(x, exp), r
    return out


@pytest.mark.parametrize("switch", [{}, {"MPJX_P2P_POOL": "0"}, {"MPJX_P2P_BATCH": "0"}], ids=["pool", "pool_off", "batch_off"])
def test_halo_2x2_persistent_agrees_with_isend_irecv(halo_reference, switch):
    out, stats = halo(True, **switch)
    for r in range(4):
        assert out[r][0] == halo_reference[r][0], (r, "tile")
        assert out[r][1] == halo_reference[r][1], (r, "indexed side buffer")
    if switch:
        assert all(s[:4] == (0, 0, 0, 0) for s in stats), stats  # the switch keeps every batch on the table path
    else:
        assert sum(s[1] for s in stats) >= 1 and all(0 <= s[3] <= SLOTS for s in stats), stats


# ---- 4. one launch above the old cap -------------------------------------------------------------------------------

def many_pairs(c, npairs, iters, mover=0, plain_at=None):
    """npairs messages of 8 B between two ranks (message k goes 0 -> 1 for even k, 1 -> 0 for odd k), persistent,
    `iters` iterations in the fixed order. Per iteration: the deltas of (p2p launches, pool launches, puts, hits) on
    this rank, slots in use, and whether the received buffer is right. plain_at: that pair goes through Isend /
    Irecv instead."""
    me, other = c.Rank(), 1 - c.Rank()
    s = torch.zeros(npairs * 4, dtype=torch.int32, device="cuda")
    r = torch.full((npairs * 4,), -1, dtype=torch.int32, device="cuda")
    base = torch.arange(npairs * 4, dtype=torch.int32, device="cuda")
    req, plain = [], []
    for k in range(npairs):
        if k == plain_at:
            continue
        if k % 2 == me:
            req.append(c.Send_init(s, 4 * k + 1, 2, MPI.INT, other, k))
        else:
            req.append(c.Recv_init(r, 4 * k + 1, 2, MPI.INT, other, k))

    def start():
        if plain_at is not None:
            k = plain_at
            plain[:] = [c.Isend(s, 4 * k + 1, 2, MPI.INT, other, k) if k % 2 == me else c.Irecv(r, 4 * k + 1, 2, MPI.INT, other, k)]
        Prequest.Startall(req)

    rows = []
    for it in range(iters):
        s.copy_(base + 1000 * me + 7 * it)
        r.fill_(-1)
        before = (c.p2p_stats()[0],) + c.p2p_pool_stats()[:3]
        ordered(c, mover, start, lambda: Request.Waitall(req + plain))
        after = (c.p2p_stats()[0],) + c.p2p_pool_stats()[:3]
        exp = np.full(4 * npairs, -1, np.int32)
        for k in range(npairs):
            if k % 2 != me:
                exp[4 * k + 1:4 * k + 3] = np.arange(4 * k + 1, 4 * k + 3) + 1000 * other + 7 * it
        rows.append((tuple(a - b for a, b in zip(after, before)), c.p2p_pool_stats()[3], np.array_equal(host(r), exp)))
        assert inactive(req)
    for q in req:
        q.Free()
    return rows


@pytest.mark.parametrize("npairs,table_launches,pool_launches", [(30, 2, 1), (513, 22, 2)])
def test_one_pool_launch_moves_more_pairs_than_a_table_holds(npairs, table_launches, pool_launches):
    comms = world(2)
    assert comms[0].p2p_stats()[3] == 24 and comms[0].p2p_pool_stats()[4] == BATCH_MAX
    out = H.run_ranks(comms, lambda c: many_pairs(c, npairs, 3))
    mover, peer = out
    # iteration 1: the table path (24 segments per launch), then every segment is stored
    assert mover[0] == ((table_launches, 0, npairs, 0), npairs, True), mover[0]
    # iterations 2 and 3: the whole batch from the pool
    for it in (1, 2):
        assert mover[it] == ((pool_launches, pool_launches, 0, npairs), npairs, True), (it, mover[it])
    assert [row for row in peer] == [((0, 0, 0, 0), 0, True)] * 3, peer
    free(comms)


# ---- 5. tile boundaries, 6. the streaming form -----------------------------------------------------------------------

def boundary_cases():
    """(name, send type factory, send items, recv type factory, recv items, packed bytes, src offset, dst offset)
    over BYTE buffers; the offsets are from 256-B aligned origins."""
    by = MPI.BYTE
    cases = [("1B", None, 1, None, 1, 1, 0, 0),
             ("16KiB+48@1,2", None, 16 * 1024 + 48, None, 16 * 1024 + 48, 16 * 1024 + 48, 1, 2),
             ("granules1025", lambda: Datatype.Vector(1025, 4, 8, by), 1, None, 4100, 4100, 0, 16)]
    for glog in range(5):
        g = 1 << glog
        cases.append((f"glog{glog}", lambda g=g: Datatype.Vector(37, g, 3 * g, by), 1, None, 37 * g, 37 * g, 0, 16 * 3))
    return cases


def test_pooled_segments_at_tile_boundaries():
    comms = world(2)
    cases = boundary_cases()

    def body(c):
        me = c.Rank()
        types, req, bufs = [], [], []
        rng = np.random.default_rng(5)
        for k, (name, sty, sitems, rty, ritems, nbytes, so, do) in enumerate(cases):
            st = sty() if sty else MPI.BYTE
            rt = rty() if rty else MPI.BYTE
            types += [t for t in (st, rt) if t is not MPI.BYTE]
            span = 256 + max(st.Extent() * sitems, rt.Extent() * ritems) + 256
            buf = torch.full((span,), 0xA5, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 256 == 0
            bufs.append(buf)
            if me == 1:
                req.append(c.Send_init(buf, 256 + so, sitems, st, 0, k))
            else:
                req.append(c.Recv_init(buf, 256 + do, ritems, rt, 1, k))
        ok = []
        for it in range(2):  # 0: the table path and the puts; 1: the pool
            src = [rng.integers(0, 256, b.numel(), dtype=np.uint8) for b in bufs]
            for b, a in zip(bufs, src):
                b.copy_(dev(a) if me == 1 else torch.full_like(b, 0xA5))
            before = c.p2p_pool_stats()
            ordered(c, 0, lambda: Prequest.Startall(req), lambda: Request.Waitall(req))
            after = c.p2p_pool_stats()
            if me == 0:
                assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == ((0, len(cases), 0), (1, 0, len(cases)))[it]
                for k, (name, sty, sitems, rty, ritems, nbytes, so, do) in enumerate(cases):
                    exp = np.full(bufs[k].numel(), 0xA5, np.uint8)
                    if sty:  # Vector(n, g, stride): n blocks of g bytes, stride bytes apart
                        n, g, stride = (1025, 4, 8) if name.startswith("granules") else (37, nbytes // 37, 3 * (nbytes // 37))
                        sel = PC.blocks([g] * n, [stride * j for j in range(n)])
                    else:
                        sel = np.arange(nbytes)
                    exp[256 + do:256 + do + nbytes] = src[k][256 + so + sel]
                    bad = PC.differs(host(bufs[k]), exp, f"{name} iteration {it}")
                    assert bad is None, bad
                    ok.append(name)
        for q in req:
            q.Free()
        for t in types:
            t.Free()
        return ok
    out = H.run_ranks(comms, body)
    assert len(out[0]) == 2 * len(cases)
    free(comms)


def test_pooled_streaming_form():
    """Two pooled contiguous messages of kStridedStreamBytes / 2 each: the batch's payload reaches the streaming
    threshold, so the second iteration is k_msgs_pool<NT>. Compared on the device."""
    comms = world(2)
    half = STREAM_BYTES // 2

    def body(c):
        me = c.Rank()
        bufs = [torch.zeros(half // 8, dtype=torch.int64, device="cuda") for _ in range(2)]
        req = [(c.Send_init if me == 1 else c.Recv_init)(b, 0, half // 8, MPI.LONG, 1 - me, k) for k, b in enumerate(bufs)]
        same = []
        for it in range(2):
            for k, b in enumerate(bufs):
                if me == 1:
                    torch.arange(half // 8, dtype=torch.int64, device="cuda", out=b)
                    b.mul_(it + 3).add_(k)
                else:
                    b.fill_(-1)
            before = c.p2p_pool_stats()
            ordered(c, 0, lambda: Prequest.Startall(req), lambda: Request.Waitall(req))
            after = c.p2p_pool_stats()
            if me == 0:
                assert (after[0] - before[0], after[2] - before[2]) == ((0, 0), (1, 2))[it]
                for k, b in enumerate(bufs):
                    exp = torch.arange(half // 8, dtype=torch.int64, device="cuda").mul_(it + 3).add_(k)
                    same.append(bool(torch.equal(b, exp)))
                    del exp
        for q in req:
            q.Free()
        return same
    out = H.run_ranks(comms, body, limit=90)
    assert out[0] == [True] * 4
    free(comms)


# ---- 7. subsets and wildcards ----------------------------------------------------------------------------------------

def test_waitall_entered_with_two_of_four_pairs_matched():
    comms = world(2)

    def body(c):
        me = c.Rank()
        s = dev(np.arange(64, dtype=np.int32))
        r = torch.full((64,), -1, dtype=torch.int32, device="cuda")
        req = [(c.Send_init(s, 16 * k, 5, MPI.INT, 0, k) if me == 1 else c.Recv_init(r, 16 * k + 1, 5, MPI.INT, 1, k))
               for k in range(4)]
        ordered(c, 0, lambda: Prequest.Startall(req), lambda: Request.Waitall(req))  # all four into rank 0's pool
        r.fill_(-1)
        s.add_(1000)
        before = c.p2p_pool_stats()  # this rank's own, read from its own thread
        base = pool_hits(comms[0])
        if me == 1:
            Prequest.Startall(req[:2])
        c.Barrier()
        if me == 0:
            Prequest.Startall(req)
            Request.Waitall(req)  # entered with pairs 0 and 1 matched: they go first, the rest when it arrives
            got = c.p2p_pool_stats()
            out = (got[0] - before[0], got[1] - before[1], got[2] - before[2], host(r).tolist())
        else:
            deadline = time.monotonic() + 20
            for want, start in ((2, req[2:]), (4, [])):  # rank 0 moves the first two, then the other two
                while pool_hits(comms[0]) < base + want:
                    assert time.monotonic() < deadline, f"rank 0 did not move {want} pairs from its pool in 20 s"
                    time.sleep(0)
                Prequest.Startall(start)
            Request.Waitall(req)  # this rank claims nothing: rank 0 has moved all four
            out = None
        c.Barrier()
        for q in req:
            q.Free()
        return out
    launches, puts, hits, data = H.run_ranks(comms, body)[0]
    assert (launches, puts, hits) == (2, 0, 4), (launches, puts, hits)  # the first two apart from the rest
    exp = np.full(64, -1, np.int32)
    for k in range(4):
        exp[16 * k + 1:16 * k + 6] = np.arange(16 * k, 16 * k + 5) + 1000
    assert data == exp.tolist()
    free(comms)


def test_any_source_receive_gets_a_slot_per_sender():
    comms = world(3)

    def body(c):
        me = c.Rank()
        buf = dev(np.full(8, 100 * me, np.int32)) if me else torch.full((8,), -1, dtype=torch.int32, device="cuda")
        req = c.Recv_init(buf, 0, 8, MPI.INT, MPI.ANY_SOURCE, MPI.ANY_TAG) if me == 0 else c.Send_init(buf, 0, 8, MPI.INT, 0, 10 + me)
        seen = []
        for it in range(4):
            sender = 1 + it % 2
            mine = [req] if me in (0, sender) else []
            if me == sender:
                buf.fill_(100 * me + it)
            st = ordered(c, 0, lambda: Prequest.Startall(mine), lambda: Request.Waitall(mine))
            if me == 0:
                seen.append((triple(st[0]), host(buf).tolist() == [100 * sender + it] * 8, c.p2p_pool_stats()[1:4]))
        req.Free()
        return seen
    seen = H.run_ranks(comms, body)[0]
    assert [s[0] for s in seen] == [(1, 11, 8), (2, 12, 8), (1, 11, 8), (2, 12, 8)] and all(s[1] for s in seen)
    # (puts, hits, slots in use) after each iteration: each (sender, receiver) pair has its own slot
    assert [s[2] for s in seen] == [(1, 0, 1), (2, 0, 2), (2, 1, 2), (2, 2, 2)]
    free(comms)


def test_short_message_proc_null_and_count_zero():
    comms = world(2)

    def body(c):
        me, other = c.Rank(), 1 - c.Rank()
        s = dev(np.arange(8, dtype=np.int32) + 50 * me)
        r = torch.full((12,), -1, dtype=torch.int32, device="cuda")
        req = [c.Recv_init(r, 2, 8, MPI.INT, other, 0),            # room for 8, the message has 3
               c.Send_init(s, 1, 3, MPI.INT, other, 0),
               c.Recv_init(r, 0, 4, MPI.INT, MPI.PROC_NULL, 1),
               c.Send_init(s, 0, 4, MPI.INT, MPI.PROC_NULL, 1),
               c.Recv_init(r, 0, 0, MPI.INT, other, 2),            # count 0
               c.Send_init(None, 0, 0, MPI.INT, other, 2)]
        res = []
        for it in range(3):
            r.fill_(-1)
            s.add_(1)
            sts = ordered(c, 0, lambda: Prequest.Startall(req), lambda: Request.Waitall(req))
            exp = np.full(12, -1, np.int32)
            exp[2:5] = np.arange(1, 4) + 50 * other + it + 1
            res.append(([triple(x) for x in sts], host(r).tolist() == exp.tolist(), inactive(req)))
        hits = c.p2p_pool_stats()[2]
        for q in req:
            q.Free()
        return res, hits
    out = H.run_ranks(comms, body)
    for me in range(2):
        for sts, data_ok, idle in out[me][0]:
            assert sts == [(1 - me, 0, 3), EMPTY, EMPTY, EMPTY, (1 - me, 2, 0), EMPTY], sts
            assert data_ok and idle
    assert out[0][1] == 4  # the two 12-B messages, from the pool in iterations 2 and 3; empty ones move nothing
    free(comms)


# ---- 8. mixed and stale ---------------------------------------------------------------------------------------------

def test_a_plain_pair_in_the_batch_takes_the_table_path():
    comms = world(2)
    out = H.run_ranks(comms, lambda c: many_pairs(c, 6, 3, plain_at=3))
    # iteration 1 stores the five persistent pairs; afterwards the plain pair keeps the whole batch on the table path
    assert [row[0] for row in out[0]] == [(1, 0, 5, 0), (1, 0, 0, 0), (1, 0, 0, 0)], out[0]
    assert all(row[2] for row in out[0] + out[1])
    free(comms)


def test_a_freed_receive_leaves_no_stale_slot():
    comms = world(2)

    def body(c):
        me = c.Rank()
        s = dev(np.arange(1, 9, dtype=np.int32))
        r = torch.full((32,), -1, dtype=torch.int32, device="cuda")
        vec = Datatype.Vector(8, 1, 3, MPI.INT)
        rs = c.Send_init(s, 0, 8, MPI.INT, 0, 0) if me == 1 else None
        rr = c.Recv_init(r, 0, 8, MPI.INT, 1, 0) if me == 0 else None
        got = []
        for it in range(4):
            if it == 2 and me == 0:  # the same buffer, another layout: a new request, a new serial, a new segment
                rr.Free()
                rr = c.Recv_init(r, 1, 1, vec, 1, 0)
            r.fill_(-1)
            mine = [rs if me == 1 else rr]
            ordered(c, 0, lambda: Prequest.Startall(mine), lambda: Request.Waitall(mine))
            got.append((host(r).tolist(), c.p2p_pool_stats()[1:4]))
        mine[0].Free()
        vec.Free()
        return got
    got = H.run_ranks(comms, body)[0]
    flat = [-1] * 32
    flat[0:8] = range(1, 9)
    strided = [-1] * 32
    strided[1:1 + 24:3] = range(1, 9)
    assert [g[0] for g in got] == [flat, flat, strided, strided]
    assert [g[1][:2] for g in got] == [(1, 0), (1, 1), (2, 1), (2, 2)]  # (puts, hits): the new pair is stored anew
    assert all(g[1][2] <= 2 for g in got)
    free(comms)


def test_a_full_pool_falls_back_to_the_table_path():
    comms = world(2)
    n = SLOTS + 6
    out = H.run_ranks(comms, lambda c: many_pairs(c, n, 2), limit=90)
    (d0, used0, ok0), (d1, used1, ok1) = out[0]
    assert ok0 and ok1 and all(row[2] for row in out[1])
    assert d0[1:] == (0, SLOTS, 0) and used0 == SLOTS      # as many segments stored as there are slots
    assert d1[1:] == (0, 0, 0) and used1 == SLOTS          # six pairs are not pooled: the batch takes the table path
    assert d0[0] == d1[0] == (n + 23) // 24
    free(comms)


# ---- 9. errors ----------------------------------------------------------------------------------------------------------

def test_start_errors_post_nothing():
    comms = world(2)

    def body(c):
        me, other = c.Rank(), 1 - c.Rank()
        s = dev(np.full(4, me + 1, np.int32))
        r = torch.zeros(4, dtype=torch.int32, device="cuda")
        rr, rs = c.Recv_init(r, 0, 4, MPI.INT, other, 0), c.Send_init(s, 0, 4, MPI.INT, other, 0)
        plain = c.Irecv(r, 0, 4, MPI.INT, other, 99)
        # Startall with one plain handle in the list: nothing posted, every request still inactive
        with pytest.raises(MPIException, match=r"\(-1\).*not a persistent request"):
            Prequest.Startall([rr, plain, rs])
        assert inactive([rr, rs])
        with pytest.raises(MPIException, match=r"\(-1\)"):
            Prequest.Startall([rr, rr])
        assert inactive([rr, rs])
        rr.Start()
        with pytest.raises(MPIException, match=r"\(-1\).*is active"):  # Start on an active request
            rr.Start()
        with pytest.raises(MPIException, match=r"\(-1\).*is active"):
            Prequest.Startall([rs, rr])
        assert rr.Is_active() and not rs.Is_active()
        c.Barrier()
        rs.Start()
        st = Request.Waitall([rr, rs])[0]
        c.Barrier()
        # exactly one message arrived under tag 0; the plain receive is still unmatched
        plain.Free()
        for q in (rr, rs):
            q.Free()
        with pytest.raises(MPIException, match=r"\(-1\)"):
            rr.Start()  # freed: a NULL handle
        return triple(st), host(r).tolist()
    out = H.run_ranks(comms, body)
    assert out == [((1, 0, 4), [2] * 4), ((0, 0, 4), [1] * 4)]
    free(comms)


def test_init_and_start_argument_errors():
    """The argument errors that need a world: a bad rank, a freed type, NULL with a nonzero count, mpjx_start on a
    handle of mpjx_irecv; and, on a live communicator, the ones tests/test_preq_abi.py checks without a device.
    Nothing is posted and the world stays usable."""
    import ctypes

    from mpjexpress_amd import _lib
    comms = world(2)
    L, c = _lib.lib(), comms[0]
    torch.cuda.set_device(0)
    buf = torch.zeros(8, dtype=torch.int32, device="cuda")
    vec = Datatype.Vector(2, 1, 2, MPI.INT)
    vec.Free()
    for bad, msg in ((lambda: c.Send_init(buf, 0, 1, MPI.INT, 2, 0), "out of range"),
                     (lambda: c.Recv_init(buf, 0, 1, MPI.INT, -1, 0), "out of range"),
                     (lambda: c.Send_init(buf, 0, 1, MPI.INT, MPI.ANY_SOURCE, 0), "out of range"),
                     (lambda: c.Send_init(buf, 0, 1, MPI.INT, 1, -1), "negative"),
                     (lambda: c.Send_init(buf, 0, 1, MPI.INT, 1, MPI.ANY_TAG), "negative"),
                     (lambda: c.Recv_init(buf, 0, 1, MPI.INT, 1, -1), "negative"),
                     (lambda: c.Send_init(buf, 0, 1, vec, 1, 0), "freed datatype")):
        with pytest.raises(MPIException, match=r"\(-1\).*" + msg):
            bad()
    h = ctypes.c_void_p()
    for init in (L.mpjx_send_init, L.mpjx_recv_init):
        assert init(c.handle, buf.data_ptr(), 1, 5, 1, 0, None) == -1                      # NULL request
        assert init(c.handle, buf.data_ptr(), -1, 5, 1, 0, ctypes.byref(h)) == -1 and not h.value  # negative count
        assert init(c.handle, None, 4, 5, 1, 0, ctypes.byref(h)) == -1 and not h.value     # NULL with a nonzero count
    plain = c.Irecv(buf, 0, 4, MPI.INT, 1, 0)
    hp = ctypes.c_void_p(plain._h.value)
    assert L.mpjx_start(ctypes.byref(hp)) == -1 and b"not a persistent request" in L.mpjx_last_error()
    assert hp.value == plain._h.value  # the handle is left as it was
    plain.Free()
    assert comms[0].p2p_pool_stats()[:4] == (0, 0, 0, 0) and comms[0].p2p_stats()[:3] == (0, 0, 0)
    assert H.run_ranks(comms, lambda k: k.Barrier() or True) == [True, True]
    free(comms)


def test_base_type_mismatch_fails_both_and_both_start_again():
    comms = world(2)

    def body(c):
        me = c.Rank()
        buf = torch.full((8,), -1, dtype=torch.int32, device="cuda") if me == 0 else dev(np.ones(8, np.float32))
        req = c.Recv_init(buf, 0, 8, MPI.INT, 1, 9) if me == 0 else c.Send_init(buf, 0, 8, MPI.FLOAT, 0, 9)
        msgs = []
        for it in range(2):  # startable again after the failure (and it fails again: the types have not changed)
            req.Start()
            try:
                req.Wait()
                msgs.append("returned")
            except MPIException as e:
                msgs.append(str(e))
            assert inactive([req])
            c.Barrier()
        untouched = me == 1 or bool((host(buf) == -1).all())
        req.Free()
        # the world is still usable
        s, r = dev(np.full(4, me + 1, np.int32)), torch.zeros(4, dtype=torch.int32, device="cuda")
        c.Sendrecv(s, 0, 4, MPI.INT, 1 - me, 0, r, 0, 4, MPI.INT, 1 - me, 0)
        return msgs, untouched, host(r).tolist()
    out = H.run_ranks(comms, body)
    for me, (msgs, untouched, data) in enumerate(out):
        for m in msgs:
            assert "(-1)" in m and "base type" in m and "send(rank 1 -> 0" in m and "recv(rank 0 <- 1" in m, m
        assert untouched and data == [2 - me] * 4
    free(comms)


def test_a_peer_that_never_starts_times_out_and_fails_the_world():
    comms = world(2, timeout=0.5)

    def body(c):
        me = c.Rank()
        buf = torch.zeros(4, dtype=torch.int32, device="cuda")
        req = c.Recv_init(buf, 0, 4, MPI.INT, 1, 3) if me == 0 else c.Send_init(buf, 0, 4, MPI.INT, 0, 3)
        first = "not started"
        if me == 0:
            req.Start()
            try:
                req.Wait()
                first = "returned"
            except MPIException as e:
                first = str(e)
            assert inactive([req])
        deadline = time.monotonic() + 20
        second = None
        while second is None and time.monotonic() < deadline:  # rank 1 sees the failed world once rank 0 gave up
            try:
                if me == 0:
                    req.Start()
                    second = "started"
                else:
                    c.Send_init(buf, 0, 4, MPI.INT, 0, 3).Free()  # posts nothing: rank 0's receive stays unmatched
            except MPIException as e:
                second = str(e)
        req.Free()
        return first, second
    out = H.run_ranks(comms, body, limit=40)
    assert "(-7)" in out[0][0] and "timed out" in out[0][0] and "recv(rank 0 <- 1, tag 3" in out[0][0], out[0][0]
    assert out[0][1] and "(-7)" in out[0][1] and out[1][1] and "(-7)" in out[1][1], out
    free(comms)


def test_send_init_in_an_rccl_world_is_unsupported():
    """A stand-in RCCL world needs another build of the library, so it runs in a process of its own."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "preq_standin_worker.py")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and "PREQ STANDIN OK" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
