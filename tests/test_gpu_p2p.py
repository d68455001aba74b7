"""GPU: Send, Recv, Isend, Irecv, Sendrecv, Sendrecv_replace, Wait, Test and Waitall on device buffers, with rank
threads in-process on device 0 (P = 1 .. 4). Expected bytes come from numpy indexing of the layouts
(tests/p2p_cases.py); every receive buffer starts as a sentinel and is compared whole, padding included; send
buffers must come back unchanged. The reference's known answers (test/mpi/pt2pt, test/mpi/dtyp/Vector.java) are
data in tests/golden/pt2pt_kat.json."""
import threading
import time

import numpy as np
import pytest

import p2p_cases as PC
from mpjexpress_amd import mpi
from mpjexpress_amd.mpi import MPI, Datatype, MPIException, Request

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LENGTHS = (0, 1, 15, 16, 17, 31, 33, 4099, 70001)
ALIGN = ((0, 0), (0, 1), (3, 3), (5, 12), (15, 8))


def run_ranks(comms, fn, limit=60):
    """fn(comm) on one thread per rank under a time limit; returns (results, errors) per rank."""
    P = len(comms)
    out, err = [None] * P, [None] * P

    def body(r):
        try:
            torch.cuda.set_device(0)
            out[r] = fn(comms[r])
        except BaseException as e:  # noqa: BLE001
            err[r] = e
    ts = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(P)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=limit)
    assert not any(t.is_alive() for t in ts), "a rank hung"
    return out, err


def ok(res):
    out, err = res
    for e in err:
        if e is not None:
            raise e
    return out


def world(P, timeout=20):
    comms = mpi.smp_world(P, [0] * P)
    for c in comms:
        c.set_p2p_timeout(timeout)
    return comms


def free(comms):
    for c in comms:
        c.Free()


@pytest.fixture(scope="module", params=[2, 3, 4])
def ranks(request):
    comms = world(request.param)
    yield comms
    free(comms)


@pytest.fixture(scope="module")
def two():
    comms = world(2)
    yield comms
    free(comms)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


# ---- the reference's known answers ------------------------------------------------------------------------------

def test_kat_sendrecv_and_sendrecv_replace(ranks):
    k = PC.kat()["sendrecv"]
    n, size, P = k["count"], k["buffer"], len(ranks)

    def body(c):
        me = c.Rank()
        bad = []
        steps = []
        if me < 2:
            steps.append((1 - me, 1 - me))
        steps.append(((me - 1) % P, (me + 1) % P))
        for src, dest in steps:
            for replace in (False, True):
                send = np.zeros(size, np.int32)
                send[:n] = me
                recv = np.zeros(size, np.int32)
                recv[:n] = k["recv_init"]
                s, r = dev(send), dev(recv)
                if replace:
                    st = c.Sendrecv_replace(s, 0, n, MPI.INT, dest, me, src, src)
                    got, exp = host(s), send.copy()
                else:
                    st = c.Sendrecv(s, 0, n, MPI.INT, dest, me, r, 0, n, MPI.INT, src, src)
                    got, exp = host(r), recv.copy()
                    if not np.array_equal(host(s), send):
                        bad.append("send buffer changed")
                exp[:n] = src
                if not np.array_equal(got, exp) or (st.source, st.tag) != (src, src) or st.Get_count(MPI.INT) != n:
                    bad.append((me, src, dest, replace, st.source, st.tag))
        c.Barrier()
        return bad
    assert ok(run_ranks(ranks, body)) == [[]] * P


def test_kat_getcount_non_overtaking_and_vector(two):
    K = PC.kat()

    def body(c):
        me, bad = c.Rank(), []
        g, no, v = K["getcount"], K["non_overtaking"], K["vector"]
        ints = np.arange(g["count"], dtype=np.int32)
        a = np.arange(no["count"], dtype=np.int32) + 1
        f = np.arange(no["count"], dtype=np.float32) + 11
        data = np.arange(v["num_params"], dtype=np.float64) ** 2
        vec = Datatype.Vector(*v["vector"], MPI.DOUBLE)
        if me == 0:
            c.Send(dev(ints), 0, g["count"], MPI.INT, 1, g["tag"])
            c.Send(dev(a), 0, no["count"], MPI.INT, 1, no["first"]["tag"])
            c.Send(dev(f), 0, no["count"], MPI.FLOAT, 1, no["second"]["tag"])
            d = dev(data)
            c.Send(d, 0, v["sendcount"], vec, 1, v["tag"])
            if not np.array_equal(host(d), data):
                bad.append("vector send buffer changed")
        else:
            r = torch.full((g["count"] + 3,), -1, dtype=torch.int32, device="cuda")
            st = c.Recv(r, 0, g["count"], MPI.INT, 0, g["tag"])
            if st.Get_count(MPI.INT) != g["expect_count"] or not np.array_equal(host(r), np.r_[ints, [-1] * 3]):
                bad.append("getcount")
            ri = torch.full((no["count"],), no["first"]["recv_init"], dtype=torch.int32, device="cuda")
            rf = dev(np.arange(no["count"], dtype=np.float32) + 19)
            s1 = c.Recv(ri, 0, no["count"], MPI.INT, 0, MPI.ANY_TAG)
            s2 = c.Recv(rf, 0, no["count"], MPI.FLOAT, 0, no["second"]["recvtag"])
            if not (np.array_equal(host(ri), a) and np.array_equal(host(rf), f)) or (s1.tag, s2.tag) != (999, 992):
                bad.append("non_overtaking")
            rd = torch.full((v["num_params"],), -7.0, dtype=torch.float64, device="cuda")
            st = c.Recv(rd, 0, v["recvcount"], MPI.DOUBLE, 0, v["tag"])
            exp = np.full(v["num_params"], -7.0)
            exp[:64] = (16.0 * np.arange(64)) ** 2
            if not np.array_equal(host(rd), exp) or st.Get_count(MPI.DOUBLE) != 64 or st.Get_count(vec) != 1:
                bad.append("vector")
        c.Barrier()
        vec.Free()
        return bad
    assert ok(run_ranks(two, body)) == [[], []]


def test_kat_wildcard_and_waitall(ranks):
    P = len(ranks)

    def body(c):
        me, bad = c.Rank(), []
        # wildcard.java: ANY_SOURCE from P - 1 senders, any arrival order, each message exactly once
        if me == 0:
            seen = set()
            for _ in range(P - 1):
                val = torch.full((3,), -1, dtype=torch.int32, device="cuda")
                st = c.Recv(val, 1, 1, MPI.INT, MPI.ANY_SOURCE, 0)
                got = host(val)
                if got[1] != st.source * 1000 + st.tag or got[0] != -1 or got[2] != -1 or st.Get_count(MPI.INT) != 1:
                    bad.append(("wildcard", got.tolist(), st.source, st.tag))
                seen.add(st.source)
            if seen != set(range(1, P)):
                bad.append(("wildcard sources", sorted(seen)))
        else:
            c.Send(dev(np.array([me * 1000], np.int32)), 0, 1, MPI.INT, 0, 0)
        c.Barrier()
        # waitall.java
        mebuf = dev(np.array([me], np.int32))
        data = torch.full((P,), -1, dtype=torch.int32, device="cuda")
        req = []
        for i in range(P):
            if i != me:
                req.append(c.Isend(mebuf, 0, 1, MPI.INT, i, 1))
                req.append(c.Irecv(data, i, 1, MPI.INT, i, 1))
        sts = Request.Waitall(req)
        exp = np.arange(P, dtype=np.int32)
        exp[me] = -1
        if not np.array_equal(host(data), exp) or not all(r.Is_null() for r in req):
            bad.append(("waitall", host(data).tolist()))
        if [s.source for s in sts[1::2]] != [i for i in range(P) if i != me]:
            bad.append(("waitall statuses", [s.source for s in sts]))
        c.Barrier()
        return bad
    assert ok(run_ranks(ranks, body)) == [[]] * P


# ---- types, alignments, layouts ------------------------------------------------------------------------------------

def test_every_basic_and_pair_type(two):
    types = mpi.DATATYPES + [MPI.SHORT2, MPI.INT2, MPI.LONG2, MPI.FLOAT2, MPI.DOUBLE2]

    def body(c):
        me, bad = c.Rank(), []
        for dt in types:
            for n in (0, 1, 17, 4099):
                nb = n * dt.byteSize
                raw = np.random.default_rng(dt.code + n).integers(0, 256, nb + 64, dtype=np.uint8)
                td = PC.torch_dtype(torch, dt)
                if me == 0:
                    s = dev(raw).view(td)
                    c.Send(s, 0, n, dt, 1, 5)
                    if not np.array_equal(host(s.view(torch.uint8)), raw):
                        bad.append((dt.name, n, "send changed"))
                else:
                    r = torch.full((nb + 64,), PC.SENT, dtype=torch.uint8, device="cuda")
                    st = c.Recv(r.view(td), 0, n, dt, 0, 5)
                    exp = np.full(nb + 64, PC.SENT, np.uint8)
                    exp[:nb] = raw[:nb]
                    m = PC.differs(host(r), exp, f"{dt.name} n={n}")
                    if m or st.Get_count(dt) != n or st.Get_elements(dt) != n * dt.size:
                        bad.append(m or (dt.name, n, st.Get_count(dt)))
        c.Barrier()
        return bad
    assert ok(run_ranks(two, body)) == [[], []]


@pytest.mark.parametrize("blocking_send", [False, True])
def test_contiguous_alignment_sweep(two, blocking_send):
    """Isend + Wait moves sender -> receiver in place; Send (eager up to 128 KiB) goes through the slab."""
    raw = np.random.default_rng(3).integers(0, 256, LENGTHS[-1] + 64, dtype=np.uint8)

    def body(c):
        me, bad = c.Rank(), []
        s = dev(raw).view(torch.int8)
        r = torch.empty(LENGTHS[-1] + 64, dtype=torch.uint8, device="cuda")
        assert s.data_ptr() % 16 == 0 and r.data_ptr() % 16 == 0
        for n in LENGTHS:
            for a, b in ALIGN:
                if me == 0:
                    if blocking_send:
                        c.Send(s, a, n, MPI.BYTE, 1, n)
                    else:
                        c.Isend(s, a, n, MPI.BYTE, 1, n).Wait()
                else:
                    r.fill_(PC.SENT)
                    st = c.Recv(r.view(torch.int8), b, n, MPI.BYTE, 0, n)
                    exp = np.full(r.numel(), PC.SENT, np.uint8)
                    exp[b:b + n] = raw[a:a + n]
                    m = PC.differs(host(r), exp, f"n={n} a={a} b={b}")
                    if m or st.Get_count(MPI.BYTE) != n:
                        bad.append(m or ("count", n))
        if me == 0 and not np.array_equal(host(s.view(torch.uint8)), raw):
            bad.append("send changed")
        c.Barrier()
        return bad, c.p2p_stats()
    eager0 = two[0].p2p_stats()[2]
    out = ok(run_ranks(two, body))
    assert [o[0] for o in out] == [[], []]
    small = sum(1 for n in LENGTHS if n <= 128 << 10) * len(ALIGN)
    assert out[0][1][2] - eager0 == (small if blocking_send else 0)


@pytest.mark.parametrize("base", ["DOUBLE", "BYTE"])
def test_layout_matrix(two, base):
    """send type x receive type over the six layout kinds; the receive count is the smallest that holds the
    message, so most messages end inside the receive layout's last item."""
    bt = MPI.DOUBLE if base == "DOUBLE" else MPI.BYTE
    L = PC.layouts(bt)
    npd = bt.np_dtype

    def body(c):
        me, bad = c.Rank(), []
        tag = 0
        for sl in L:
            si = 300 if sl.name == "contiguous" else 3
            sidx = sl.indices(si)
            src = (np.arange(sl.span(si) + 5) * 3 + 1).astype(npd)
            for rl in L:
                tag += 1
                ri = -(-len(sidx) // len(rl.idx))
                ridx = rl.indices(ri)[:len(sidx)]
                if me == 0:
                    s = dev(src)
                    c.Isend(s, 2, si, sl.dt, 1, tag).Wait()
                    if not np.array_equal(host(s), src):
                        bad.append((sl.name, rl.name, "send changed"))
                else:
                    r = torch.full((rl.span(ri) + 7,), -3, dtype=PC.torch_dtype(torch, bt), device="cuda")
                    st = c.Recv(r, 3, ri, rl.dt, 0, tag)
                    exp = np.full(rl.span(ri) + 7, -3).astype(npd)
                    exp[3 + ridx] = src[2 + sidx]
                    if not np.array_equal(host(r), exp) or st.Get_elements(rl.dt) != len(sidx):
                        bad.append((sl.name, rl.name, int((host(r) != exp).sum())))
        c.Barrier()
        return bad
    assert ok(run_ranks(two, body)) == [[], []]
    for l in L[1:]:
        l.dt.Free()


def test_message_shorter_than_the_receive_layout(two):
    """7 doubles into 3 items of Vector(2, 2, 5): the message ends inside the second item."""
    vec = Datatype.Vector(2, 2, 5, MPI.DOUBLE)

    def body(c):
        if c.Rank() == 0:
            c.Send(dev(np.arange(7.0) + 1), 0, 7, MPI.DOUBLE, 1, 0)
            return None
        r = torch.full((30,), -1.0, dtype=torch.float64, device="cuda")
        st = c.Recv(r, 1, 3, vec, 0, 0)
        exp = np.full(30, -1.0)
        exp[1 + np.array([0, 1, 5, 6, 7, 8, 12])] = np.arange(7.0) + 1
        return np.array_equal(host(r), exp), st.Get_count(vec), st.Get_elements(vec), st.Get_count(MPI.DOUBLE)
    out = ok(run_ranks(two, body))
    assert out[1] == (True, MPI.UNDEFINED, 7, 7)
    vec.Free()


# ---- protocol ----------------------------------------------------------------------------------------------------

def test_head_to_head_eager_send_completes():
    comms = world(2)

    def body(c):
        other = 1 - c.Rank()
        s = dev(np.full(256, c.Rank() + 1, np.int32))
        r = torch.zeros(256, dtype=torch.int32, device="cuda")
        c.Send(s, 0, 256, MPI.INT, other, 0)  # 1 KiB: eager, returns before the peer's Recv
        c.Recv(r, 0, 256, MPI.INT, other, 0)
        return int(host(r)[0]), int(host(r)[-1]), c.p2p_stats()[2]
    out = ok(run_ranks(comms, body))
    assert out == [(2, 2, 1), (1, 1, 1)]
    free(comms)


def test_head_to_head_large_send_times_out_and_fails_the_world():
    """1 MiB is above the eager limit: both ranks wait in Send for a Recv that is never posted. A host wait with
    nothing enqueued on the GPU; it ends at the 2 s limit with MPJX_ERR_INTERNAL on both ranks."""
    comms = world(2, timeout=2)

    def body(c):
        other = 1 - c.Rank()
        s = torch.zeros(1 << 18, dtype=torch.int32, device="cuda")
        t0 = time.monotonic()
        try:
            c.Send(s, 0, 1 << 18, MPI.INT, other, 0)
            first = "returned"
        except MPIException as e:
            first = str(e)
        dt = time.monotonic() - t0
        try:
            c.Recv(s, 0, 1, MPI.INT, other, 0)
            second = "returned"
        except MPIException as e:
            second = str(e)
        return first, dt, second
    out = ok(run_ranks(comms, body, limit=30))
    for first, dt, second in out:
        assert "(-7)" in first and "send(rank" in first and dt < 10, (first, dt)
        assert "(-7)" in second, second
    assert sum("timed out" in o[0] for o in out) >= 1
    free(comms)
    # the process stays healthy: a new world works
    comms = world(2)
    assert ok(run_ranks(comms, lambda c: c.Sendrecv(dev(np.ones(4, np.int32)), 0, 4, MPI.INT, 1 - c.Rank(), 0,
                                                      torch.zeros(4, dtype=torch.int32, device="cuda"), 0, 4, MPI.INT,
                                                      1 - c.Rank(), 0).source)) == [1, 0]
    free(comms)


def test_cross_order_wait_send_before_wait_recv(two):
    def body(c):
        other = 1 - c.Rank()
        s = dev(np.full(1 << 16, c.Rank() + 7, np.int32))  # 256 KiB: not eager either way
        r = torch.zeros(1 << 16, dtype=torch.int32, device="cuda")
        rs = c.Isend(s, 0, 1 << 16, MPI.INT, other, 3)
        rr = c.Irecv(r, 0, 1 << 16, MPI.INT, other, 3)
        rs.Wait()
        st = rr.Wait()
        return bool((host(r) == other + 7).all()), st.source
    assert ok(run_ranks(two, body)) == [(True, 1), (True, 0)]


def test_test_makes_progress_and_never_blocks(two):
    def body(c):
        other = 1 - c.Rank()
        r = torch.zeros(8, dtype=torch.int32, device="cuda")
        rr = c.Irecv(r, 0, 8, MPI.INT, other, 1)
        first = rr.Test()  # nothing sent yet on at least one rank: returns at once either way
        c.Barrier()
        rs = c.Isend(dev(np.full(8, c.Rank(), np.int32)), 0, 8, MPI.INT, other, 1)
        st, spins = None, 0
        while st is None and spins < 200000:
            st = rr.Test()
            spins += 1
        rs.Wait()
        return first is None, st is not None and st.source == other, host(r).tolist() == [other] * 8
    assert ok(run_ranks(two, body)) == [(True, True, True)] * 2


def test_truncation_and_base_type_mismatch(two):
    def body(c):
        me, other, res = c.Rank(), 1 - c.Rank(), []
        for what in ("truncation", "mismatch"):
            r = torch.full((16,), -1, dtype=torch.int32, device="cuda")
            try:
                if me == 0:
                    if what == "truncation":
                        c.Isend(dev(np.ones(16, np.int32)), 0, 16, MPI.INT, 1, 9).Wait()
                    else:
                        c.Isend(dev(np.ones(8, np.float32)), 0, 8, MPI.FLOAT, 1, 9).Wait()
                else:
                    c.Recv(r, 0, 8, MPI.INT, 0, 9)
                res.append("returned")
            except MPIException as e:
                res.append(str(e))
            res.append(bool((host(r) == -1).all()))
            c.Barrier()  # the world is still usable
        s = dev(np.full(4, me + 1, np.int32))
        r = torch.zeros(4, dtype=torch.int32, device="cuda")
        c.Sendrecv(s, 0, 4, MPI.INT, other, 0, r, 0, 4, MPI.INT, other, 0)
        res.append(host(r).tolist())
        return res
    out = ok(run_ranks(two, body))
    for me, res in enumerate(out):
        assert "(-1)" in res[0] and "longer than the receive layout" in res[0] and "send(rank 0 -> 1" in res[0], res[0]
        assert "recv(rank 1 <- 0" in res[0] and res[1] is True
        assert "(-1)" in res[2] and "base type" in res[2] and res[3] is True
        assert res[4] == [2 - me] * 4


def test_argument_errors_post_nothing_and_keep_the_world(two):
    c = two[0]
    torch.cuda.set_device(0)
    buf = torch.zeros(8, dtype=torch.int32, device="cuda")
    vec = Datatype.Vector(2, 1, 2, MPI.INT)
    vec.Free()
    for bad in (lambda: c.Isend(buf, 0, 1, MPI.INT, 2, 0), lambda: c.Isend(buf, 0, 1, MPI.INT, 1, -1),
                lambda: c.Irecv(buf, 0, 1, MPI.INT, -1, 0), lambda: c.Isend(buf, 0, 1, vec, 1, 0),
                lambda: c.Isend(None, 0, 0, MPI.INT, MPI.ANY_SOURCE, 0)):
        with pytest.raises(MPIException, match=r"\(-1\)"):
            bad()
    import ctypes
    from mpjexpress_amd import _lib
    h = ctypes.c_void_p()
    assert _lib.lib().mpjx_isend(c.handle, None, 4, 5, 1, 0, ctypes.byref(h)) == -1  # NULL with a nonzero count
    assert _lib.lib().mpjx_isend(c.handle, buf.data_ptr(), -1, 5, 1, 0, ctypes.byref(h)) == -1
    # PROC_NULL completes at once
    st = c.Recv(buf, 0, 4, MPI.INT, MPI.PROC_NULL, 5)
    assert (st.source, st.tag, st.Get_count(MPI.INT)) == (MPI.PROC_NULL, MPI.ANY_TAG, 0)
    c.Send(buf, 0, 4, MPI.INT, MPI.PROC_NULL, 5)
    assert ok(run_ranks(two, lambda k: k.Barrier() or True)) == [True, True]


def test_self_message_at_p1():
    comms = world(1)
    c = comms[0]
    torch.cuda.set_device(0)
    vec = Datatype.Vector(4, 1, 3, MPI.DOUBLE)
    src = np.arange(12.0)
    s = dev(src)
    r = torch.full((6,), -1.0, dtype=torch.float64, device="cuda")
    rr = c.Irecv(r, 1, 4, MPI.DOUBLE, 0, MPI.ANY_TAG)
    rs = c.Isend(s, 0, 1, vec, 0, 4)
    sts = Request.Waitall([rr, rs])
    assert host(r).tolist() == [-1.0, 0.0, 3.0, 6.0, 9.0, -1.0] and (sts[0].source, sts[0].tag) == (0, 4)
    assert np.array_equal(host(s), src)
    c.Send(s, 0, 2, MPI.DOUBLE, 0, 1)  # eager: returns, then the receive matches it
    c.Recv(r, 0, 2, MPI.DOUBLE, 0, 1)
    assert host(r).tolist()[:2] == [0.0, 1.0]
    # layouts that share a byte: MPJX_ERR_ARG on both requests, nothing moved
    rr = c.Irecv(s, 2, 4, MPI.DOUBLE, 0, 7)
    rs = c.Isend(s, 0, 4, MPI.DOUBLE, 0, 7)
    with pytest.raises(MPIException, match=r"\(-1\).*share a byte"):
        Request.Waitall([rr, rs])
    assert np.array_equal(host(s), src)
    vec.Free()
    free(comms)


def test_sendrecv_replace_on_a_vector(ranks):
    P = len(ranks)
    vec = Datatype.Vector(5, 2, 4, MPI.INT)
    idx = PC.blocks([2] * 5, [4 * j for j in range(5)])

    def body(c):
        me = c.Rank()
        src, dest = (me - 1) % P, (me + 1) % P
        mine = np.arange(40, dtype=np.int32) + 100 * me
        b = dev(mine)
        st = c.Sendrecv_replace(b, 1, 2, vec, dest, 2, src, 2)
        exp = mine.copy()
        at = 1 + np.r_[idx, idx + 18]
        exp[at] = (np.arange(40, dtype=np.int32) + 100 * src)[at]
        return np.array_equal(host(b), exp), st.source, st.Get_count(vec)
    assert ok(run_ranks(ranks, body)) == [(True, (r - 1) % P, 2) for r in range(P)]
    vec.Free()


def test_requests_of_a_destroyed_communicator_fail():
    comms = world(2)
    torch.cuda.set_device(0)
    buf = torch.zeros(4, dtype=torch.int32, device="cuda")
    rr = comms[1].Irecv(buf, 0, 4, MPI.INT, 0, 0)
    free(comms)
    with pytest.raises(MPIException, match=r"\(-7\).*destroyed"):
        rr.Wait()
    assert rr.Is_null()
