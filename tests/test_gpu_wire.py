"""GPU: MPI.PACKED messages (k_wire), Probe and Iprobe on device buffers, with P = 2 rank threads in-process on
device 0 (one P = 1 self-message) under a time limit per world. Whole receive buffers are pre-filled with a
sentinel and compared byte for byte, guard bytes past the end included.

  - pack direction (typed -> PACKED) and unpack direction (PACKED -> typed): all 14 (granule, word) arms x {linear,
    Vector, Indexed} x {1 granule, one tile, one tile + 1}; the received image against a numpy-built section AND
    mpjx_pack's image; short messages that cut a granule; the streaming form at 1 MiB
  - several sections in one message, below and above the eager limit; device-found and host-found errors; one mixed
    Waitall with exactly one k_msgs and one k_wire launch; kWireMax + 1 pairs in two launches; persistent requests;
    Probe / Iprobe
Where launch counts are asserted the order of posts and waits is fixed with barriers: the peer posts first, then ONE
rank posts and waits, claiming every pair."""
import contextlib
import os

import numpy as np
import pytest

import test_gpu_p2p_halo as H
import wire_cases as WC
from mpjexpress_amd import mpi
from mpjexpress_amd.mpi import MPI, Datatype, MPIException, Request

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PACKED = MPI.PACKED
ERR_ARG, ERR_INTERNAL = "(-1)", "(-7)"


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


def world(P=2, timeout=20, **kv):
    with env(**kv):  # the world's switches are read once, when it is created
        comms = mpi.smp_world(P, [0] * P)
    for c in comms:
        c.set_p2p_timeout(timeout)
    return comms


def free(comms):
    for c in comms:
        c.Free()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def raw(t):
    """The tensor's bytes on the host."""
    return t.cpu().numpy().view(np.uint8).reshape(-1)


def same(got, exp, what):
    got, exp = np.asarray(got).view(np.uint8).reshape(-1), np.asarray(exp).view(np.uint8).reshape(-1)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {bad[0]}: got {got[bad[0]]:#x}, expected {exp[bad[0]]:#x}"


def cases(kind):
    return [WC.Case(kind, g, w, n) for (g, w) in WC.ARMS for n in WC.LENGTHS]


# ---- 1. pack direction: typed send -> PACKED receive ---------------------------------------------------------------

@pytest.mark.parametrize("kind", WC.KINDS)
def test_pack_direction_every_arm(kind):
    comms = world()
    cs = cases(kind)

    def body(c):
        me = c.Rank()
        for k, cs_k in enumerate(cs):
            vals = cs_k.values(k)
            # the image starts 8 bytes into a 16-aligned tensor: its payload is 16-aligned, so the granule is the layout's
            total = 8 + 8 + cs_k.payload + WC.GUARD
            if me == 0:
                src = dev(vals)
                c.Isend(src, cs_k.off, cs_k.count, cs_k.dt, 1, k).Wait()
                same(raw(src), vals, f"{kind} {k}: the send buffer is only read")
            else:
                img = dev(np.full(total, WC.SENT, np.uint8))
                st = c.Recv(img, 8, 8 + cs_k.payload + 8, PACKED, 0, k)
                sec = WC.section(cs_k.base.code, vals[cs_k.off + cs_k.idx])
                what = f"{kind} glog {cs_k.glog} wlog {cs_k.wlog} ngran {cs_k.ngran}"
                same(raw(img), WC.image(total, 8, sec), what + ": numpy section")
                assert (st.source, st.tag, st.Get_count(PACKED), st.Get_elements(PACKED)) == (0, k, len(sec), len(sec)), what
                mine = dev(np.full(total, WC.SENT, np.uint8))  # mpjx_pack's image of the same buffer
                assert c.Pack(dev(vals), cs_k.off, cs_k.count, cs_k.dt, mine, 8) == 8 + len(sec)
                same(raw(img), raw(mine), what + ": mpjx_pack's image")
        return c.p2p_wire_stats()
    out = H.run_ranks(comms, body, limit=120)
    assert out[0][1] + out[1][1] == len(cs) and out[0][2] + out[1][2] == 0, out  # every pair was packed on the fly
    for x in cs:
        x.free()
    free(comms)


# ---- 2. unpack direction: PACKED send -> typed receive -------------------------------------------------------------

def short_lengths(x):
    """The full layout, and where a granule holds several words, lengths that cut one: the last granule (r = words per
    granule - 1), and the first word of a granule in the middle, across the tile boundary for the long layouts."""
    ns = [x.words]
    if x.b > 1:
        ns += [x.words - 1, (x.ngran // 2) * x.b + 1]
    return sorted(set(ns))


@pytest.mark.parametrize("kind", WC.KINDS)
def test_unpack_direction_every_arm(kind):
    comms = world()
    cs = cases(kind)

    def body(c):
        me = c.Rank()
        tag = 0
        for k, x in enumerate(cs):
            vals = x.values(1000 + k)[:x.words]  # the packed stream, in host order
            sec = WC.section(x.base.code, vals)
            for n in short_lengths(x):
                what = f"{kind} glog {x.glog} wlog {x.wlog} ngran {x.ngran} n {n}"
                if me == 0:
                    img = dev(WC.image(8 + len(sec) + WC.GUARD, 8, sec))
                    img[8:16] = dev(WC.header(x.base.code, n))  # announce n; the payload behind it stays
                    c.Isend(img, 8, 8 + n * x.w, PACKED, 1, tag).Wait()
                else:
                    dst = dev(x.blank())
                    st = c.Recv(dst, x.off, x.count, x.dt, 0, tag)
                    exp = x.blank()
                    exp[x.off + x.idx[:n]] = vals[:n]
                    same(raw(dst), exp, what)
                    assert (st.source, st.tag, st.Get_elements(x.base), st.Get_count(x.base)) == (0, tag, n, n), what
                tag += 1
        return c.p2p_wire_stats()
    out = H.run_ranks(comms, body, limit=120)
    assert out[0][2] + out[1][2] == sum(len(short_lengths(x)) for x in cs) and out[0][1] + out[1][1] == 0, out
    for x in cs:
        x.free()
    free(comms)


@pytest.mark.parametrize("base,npdt,n", [(MPI.DOUBLE, np.float64, 3), (MPI.SHORT, np.int16, 11), (MPI.BYTE, np.int8, 21)])
def test_short_message_cuts_a_granule(base, npdt, n):
    """n elements into a Vector of 16-byte blocks: n ends inside a block, which is one granule."""
    comms = world()
    w = np.dtype(npdt).itemsize
    b = 16 // w
    vec = Datatype.Vector(4, b, 2 * b, base)

    def body(c):
        vals = np.arange(1, 4 * b + 1).astype(npdt)
        if c.Rank() == 0:
            img = dev(WC.image(8 + 8 + n * w, 8, WC.section(base.code, vals[:n])))
            c.Send(img, 8, 8 + n * w, PACKED, 1, 3)  # eager: the image is copied into the slab
            torch.cuda.synchronize()  # an eager send returns before its pack has run: the buffer outlives it
            return c.p2p_stats()[2]
        dst = dev(np.full(8 * b + 4, -1, npdt))
        st = c.Recv(dst, 0, 1, vec, 0, 3)
        idx = (np.arange(4)[:, None] * 2 * b + np.arange(b)[None, :]).reshape(-1)
        exp = np.full(8 * b + 4, -1, npdt)
        exp[idx[:n]] = vals[:n]
        same(raw(dst), exp, f"{base} n {n}")
        assert st.Get_elements(base) == n and st.Get_count(vec) == MPI.UNDEFINED
        return 0
    assert H.run_ranks(comms, body) == [1, 0]
    vec.Free()
    free(comms)


# ---- 3. the streaming form -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("unpack", [False, True])
def test_streaming_form_at_1_mib(unpack):
    nblk = 65536  # blocks of 2 doubles, 3 apart: 1 MiB of payload
    vec = Datatype.Vector(nblk, 2, 3, MPI.DOUBLE)
    idx = (np.arange(nblk, dtype=np.int64)[:, None] * 3 + np.arange(2)[None, :]).reshape(-1)
    vals = np.random.default_rng(7).integers(0, 256, 3 * nblk * 8, dtype=np.uint8).view(np.float64).copy()
    with env(MPJX_STRIDED_NT_MIN_MIB=1):  # read per launch
        comms = world()

        def body(c):
            if not unpack:
                if c.Rank() == 0:
                    c.Isend(dev(vals), 0, 1, vec, 1, 1).Wait()
                else:
                    img = dev(np.full(16 + 16 * nblk + WC.GUARD, WC.SENT, np.uint8))
                    st = c.Recv(img, 8, 8 + 16 * nblk, PACKED, 0, 1)
                    same(raw(img), WC.image(len(img), 8, WC.section(8, vals[idx])), "streaming pack")
                    assert st.Get_count(PACKED) == 8 + 16 * nblk
            else:
                if c.Rank() == 0:
                    c.Isend(dev(WC.image(16 + 16 * nblk, 8, WC.section(8, vals[idx]))), 8, 8 + 16 * nblk, PACKED, 1, 1).Wait()
                else:
                    dst = dev(np.full(3 * nblk * 8, WC.SENT, np.uint8).view(np.float64))
                    st = c.Recv(dst, 0, 1, vec, 0, 1)
                    exp = np.full(3 * nblk * 8, WC.SENT, np.uint8).view(np.float64)
                    exp[idx] = vals[idx]
                    same(raw(dst), exp, "streaming unpack")
                    assert st.Get_elements(MPI.DOUBLE) == 2 * nblk
            return True
        assert H.run_ranks(comms, body) == [True, True]
        free(comms)
    vec.Free()


# ---- 4. several sections in one message --------------------------------------------------------------------------------

@pytest.mark.parametrize("eager_kib", [128, 0.0625])
def test_several_sections_in_one_message(eager_kib):
    """Pack INT x 3 and a DOUBLE Vector column into one image, send it PACKED (below and above the eager limit), Recv
    PACKED and Unpack both sections; a typed Recv(INT) of the same image gets section one only."""
    comms = world(MPJX_P2P_EAGER_KIB=eager_kib)
    col = Datatype.Vector(5, 1, 4, MPI.DOUBLE)  # a column of a 5 x 4 matrix
    ints = np.array([7, -8, 9], np.int32)
    mat = np.arange(20, dtype=np.float64) + 0.5

    def body(c):
        if c.Rank() == 0:
            img = torch.zeros(128, dtype=torch.uint8, device="cuda")
            pos = c.Pack(dev(ints), 0, 3, MPI.INT, img, 0)
            assert pos == 20
            pos = c.Pack(dev(mat), 2, 1, col, img, pos)
            assert pos == 24 + 8 + 40
            c.Send(img, 0, pos, PACKED, 1, 5)
            c.Send(img, 0, pos, PACKED, 1, 6)
            torch.cuda.synchronize()  # an eager send returns before its pack has run: the buffer outlives it
            return c.p2p_stats()[2]
        img = dev(np.full(128, WC.SENT, np.uint8))
        st = c.Recv(img, 0, 100, PACKED, 0, 5)
        assert st.Get_count(PACKED) == 72 and st.Get_elements(PACKED) == 72
        exp = np.full(128, WC.SENT, np.uint8)
        exp[0:20] = WC.section(5, ints)
        exp[20:24] = 0  # the sender's image was zeroed there
        exp[24:72] = WC.section(8, mat[2::4])
        same(raw(img), exp, "PACKED -> PACKED")
        got_i = torch.full((3,), -1, dtype=torch.int32, device="cuda")
        got_m = dev(np.full(20, -1.0))
        pos = c.Unpack(img, 0, got_i, 0, 3, MPI.INT)
        pos = c.Unpack(img, pos, got_m, 1, 1, col)
        assert pos == 72 and got_i.cpu().tolist() == [7, -8, 9]
        em = np.full(20, -1.0)
        em[1::4] = mat[2::4]
        same(raw(got_m), em, "the column")
        # a typed receive reads the first section only, and its count from the header
        got8 = torch.full((8,), -1, dtype=torch.int32, device="cuda")
        st = c.Recv(got8, 0, 8, MPI.INT, 0, 6)
        assert got8.cpu().tolist() == [7, -8, 9, -1, -1, -1, -1, -1] and st.Get_count(MPI.INT) == 3
        return 0
    assert H.run_ranks(comms, body) == [2 if eager_kib == 128 else 0, 0]
    col.Free()
    free(comms)


# ---- 5. errors -----------------------------------------------------------------------------------------------------

BAD_HEADERS = {
    "wrong type code": (WC.header(8, 3), 8 + 12, "MPJX_MPJBUF_BAD_TYPE"),
    "n above the room": (WC.header(5, 5), 8 + 20, "MPJX_MPJBUF_BAD_COUNT"),
    "n * w past the bytes sent": (WC.header(5, 3), 8 + 11, "MPJX_MPJBUF_OVERRUN"),
    "negative n": (np.array([4, 0, 0, 0, 255, 255, 255, 255], np.uint8), 8 + 12, "MPJX_MPJBUF_OVERRUN"),
}


@pytest.mark.parametrize("name", list(BAD_HEADERS))
def test_device_found_errors(name):
    hdr, sent, code = BAD_HEADERS[name]
    comms = world()

    def body(c):
        me = c.Rank()
        img = dev(np.concatenate([hdr, np.arange(1, 41, dtype=np.uint8)]))
        good = dev(WC.section(5, np.array([1, 2, 3], np.int32)))
        dst = torch.full((4,), -1, dtype=torch.int32, device="cuda")  # room: 4 INTs
        msg = None
        try:
            if me == 0:
                c.Isend(img, 0, sent, PACKED, 1, 1).Wait()  # not eager: the sender gets the error too
            else:
                c.Recv(dst, 0, 4, MPI.INT, 0, 1)
        except MPIException as e:
            msg = str(e)
        assert msg and ERR_ARG in msg and code in msg and "send(rank 0 -> 1" in msg and "recv(rank 1 <- 0" in msg, msg
        assert dst.cpu().tolist() == [-1] * 4  # untouched
        c.Barrier()
        if me == 0:  # the world stays usable: the next good message passes
            c.Send(good, 0, 20, PACKED, 1, 2)
            torch.cuda.synchronize()  # an eager send returns before its pack has run: the buffer outlives it
        else:
            st = c.Recv(dst, 0, 4, MPI.INT, 0, 2)
            assert dst.cpu().tolist() == [1, 2, 3, -1] and st.Get_count(MPI.INT) == 3
        return True
    assert H.run_ranks(comms, body) == [True, True]
    free(comms)


def test_host_found_errors():
    comms = world()

    def body(c):
        me, other = c.Rank(), 1 - c.Rank()
        ints = torch.arange(10, dtype=torch.int32, device="cuda")
        img = dev(np.full(64, WC.SENT, np.uint8))

        def fails(f, *words):
            with pytest.raises(MPIException) as e:
                f()
            assert ERR_ARG in str(e.value) and all(w in str(e.value) for w in words), str(e.value)
        # an image that is too small: 8 + 40 bytes into a room of 47; both requests fail, nothing moves
        if me == 0:
            fails(lambda: c.Isend(ints, 0, 10, MPI.INT, 1, 1).Wait(), "longer than the image of 47")
        else:
            fails(lambda: c.Recv(img, 0, 47, PACKED, 0, 1), "longer than the image of 47")
            same(raw(img), np.full(64, WC.SENT, np.uint8), "nothing moved")
        c.Barrier()
        # a PACKED send of 4 bytes to a typed receive
        if me == 0:
            fails(lambda: c.Isend(img, 0, 4, PACKED, 1, 2).Wait(), "no section header")
        else:
            dst = torch.full((4,), -1, dtype=torch.int32, device="cuda")
            fails(lambda: c.Recv(dst, 0, 4, MPI.INT, 0, 2), "no section header")
            assert dst.cpu().tolist() == [-1] * 4
        c.Barrier()
        # a misaligned image posts nothing
        fails(lambda: c.Isend(img, 4, 16, PACKED, other, 3), "8-byte aligned")
        fails(lambda: c.Irecv(img, 4, 16, PACKED, other, 3), "8-byte aligned")
        fails(lambda: c.Send_init(img, 2, 16, PACKED, other, 3), "8-byte aligned")
        c.Barrier()
        assert c.Iprobe(MPI.ANY_SOURCE, MPI.ANY_TAG) is None
        c.Barrier()
        # PACKED is a point-to-point type only
        fails(lambda: c.Pack(img, 0, 8, PACKED, dev(np.zeros(64, np.uint8)), 0), "datatype")
        # the world is still usable
        if me == 0:
            c.Send(ints, 0, 10, MPI.INT, 1, 4)
            torch.cuda.synchronize()  # an eager send returns before its pack has run: the buffer outlives it
        else:
            st = c.Recv(img, 0, 64, PACKED, 0, 4)
            assert st.Get_count(PACKED) == 48
            same(raw(img)[:48], WC.section(5, np.arange(10, dtype=np.int32)), "the next good message")
        return True
    assert H.run_ranks(comms, body) == [True, True]
    free(comms)


# ---- 6. batches ------------------------------------------------------------------------------------------------------

def test_one_mixed_waitall_is_one_k_msgs_and_one_k_wire_launch():
    """Contiguous, Vector, typed -> PACKED, PACKED -> typed and PACKED -> PACKED pairs, the peer's posted first."""
    comms = world()
    vec = Datatype.Vector(5, 3, 7, MPI.INT)
    vidx = (np.arange(5)[:, None] * 7 + np.arange(3)[None, :]).reshape(-1)
    a = np.arange(100, 140, dtype=np.int32)
    sec = WC.section(5, np.array([11, 12, 13, 14], np.int32))

    def body(c):
        me = c.Rank()
        req = []
        if me == 1:  # the senders
            bufs = [dev(a), dev(a), dev(a), dev(sec), dev(sec)]
            req.append(c.Isend(bufs[0], 0, 40, MPI.INT, 0, 0))     # contiguous -> contiguous
            req.append(c.Isend(bufs[1], 0, 1, vec, 0, 1))          # Vector -> contiguous
            req.append(c.Isend(bufs[2], 3, 1, vec, 0, 2))          # typed -> PACKED
            req.append(c.Isend(bufs[3], 0, 24, PACKED, 0, 3))      # PACKED -> typed
            req.append(c.Isend(bufs[4], 0, 24, PACKED, 0, 4))      # PACKED -> PACKED
        c.Barrier()
        before = None
        if me == 0:
            r0 = torch.full((40,), -1, dtype=torch.int32, device="cuda")
            r1 = torch.full((15,), -1, dtype=torch.int32, device="cuda")
            r2 = dev(np.full(80, WC.SENT, np.uint8))
            r3 = torch.full((35,), -1, dtype=torch.int32, device="cuda")
            r4 = dev(np.full(32, WC.SENT, np.uint8))
            torch.cuda.synchronize()
            before = (c.p2p_stats(), c.p2p_wire_stats())
            req.append(c.Irecv(r0, 0, 40, MPI.INT, 1, 0))
            req.append(c.Irecv(r1, 0, 15, MPI.INT, 1, 1))
            req.append(c.Irecv(r2, 0, 72, PACKED, 1, 2))
            req.append(c.Irecv(r3, 0, 1, vec, 1, 3))
            req.append(c.Irecv(r4, 0, 32, PACKED, 1, 4))
            sts = Request.Waitall(req)
            after = (c.p2p_stats(), c.p2p_wire_stats())
            assert after[0][0] - before[0][0] == 2 and after[0][1] - before[0][1] == 5, (before, after)
            assert [x - y for x, y in zip(after[1][:3], before[1][:3])] == [1, 1, 1], (before, after)
            assert r0.cpu().tolist() == a.tolist() and r1.cpu().tolist() == a[vidx].tolist()
            same(raw(r2), WC.image(80, 0, WC.section(5, a[3 + vidx])), "typed -> PACKED")
            e3 = np.full(35, -1, np.int32)
            e3[vidx[:4]] = [11, 12, 13, 14]
            assert r3.cpu().tolist() == e3.tolist()
            same(raw(r4), WC.image(32, 0, sec), "PACKED -> PACKED")
            assert [s.Get_count(PACKED) for s in (sts[2], sts[4])] == [68, 24] and sts[3].Get_elements(MPI.INT) == 4
        c.Barrier()
        if me == 1:
            Request.Waitall(req)
        return True
    assert H.run_ranks(comms, body) == [True, True]
    vec.Free()
    free(comms)


def test_table_max_plus_one_wire_pairs_take_two_launches():
    comms = world()

    def body(c):
        me = c.Rank()
        tmax = c.p2p_wire_stats()[3]
        n = tmax + 1
        assert tmax >= 16
        src = torch.arange(4 * n, dtype=torch.int32, device="cuda")
        imgs = dev(np.full(n * 32, WC.SENT, np.uint8))
        req = []
        if me == 1:
            req = [c.Isend(src, 4 * k, 3, MPI.INT, 0, k) for k in range(n)]
        c.Barrier()
        if me == 0:
            req = [c.Irecv(imgs, 32 * k, 24, PACKED, 1, k) for k in range(n)]
            w0, l0 = c.p2p_wire_stats(), c.p2p_stats()[0]
            Request.Waitall(req)
            w1, l1 = c.p2p_wire_stats(), c.p2p_stats()[0]
            assert (w1[0] - w0[0], w1[1] - w0[1], l1 - l0) == (2, n, 2), (w0, w1, l0, l1)
            exp = np.full(n * 32, WC.SENT, np.uint8)
            for k in range(n):
                exp[32 * k:32 * k + 20] = WC.section(5, np.arange(4 * k, 4 * k + 3, dtype=np.int32))
            same(raw(imgs), exp, "every image")
        c.Barrier()
        if me == 1:
            Request.Waitall(req)
        return True
    assert H.run_ranks(comms, body) == [True, True]
    free(comms)


def test_persistent_typed_send_packed_receive():
    comms = world()

    def body(c):
        me = c.Rank()
        src = torch.zeros(4, dtype=torch.int32, device="cuda")
        img = dev(np.full(32, WC.SENT, np.uint8))
        r = c.Send_init(src, 0, 4, MPI.INT, 1, 9) if me == 0 else c.Recv_init(img, 0, 32, PACKED, 0, 9)
        for it in range(3):
            if me == 0:
                src.copy_(torch.arange(4, dtype=torch.int32) + 10 * it)
            else:
                img.fill_(WC.SENT)
            c.Barrier()
            r.Start()
            st = r.Wait()
            if me == 1:
                same(raw(img), WC.image(32, 0, WC.section(5, np.arange(4, dtype=np.int32) + 10 * it)), f"start {it}")
                assert st.Get_count(PACKED) == 24
            c.Barrier()
        r.Free()
        return c.p2p_pool_stats()[1], c.p2p_wire_stats()[1]
    out = H.run_ranks(comms, body)
    assert out[0][0] == 0 and out[1][0] == 0 and out[0][1] + out[1][1] == 3, out  # no put: a wire pair is never pooled
    free(comms)


def test_self_message_at_p1():
    comms = world(1)

    def body(c):
        src = torch.arange(6, dtype=torch.int32, device="cuda")
        img = dev(np.full(40, WC.SENT, np.uint8))
        Request.Waitall([c.Irecv(img, 0, 40, PACKED, 0, 1), c.Isend(src, 0, 6, MPI.INT, 0, 1)])
        same(raw(img), WC.image(40, 0, WC.section(5, np.arange(6, dtype=np.int32))), "self pack")
        dst = torch.full((8,), -1, dtype=torch.int32, device="cuda")
        sts = Request.Waitall([c.Irecv(dst, 0, 8, MPI.INT, 0, 2), c.Isend(img, 0, 32, PACKED, 0, 2)])
        assert dst.cpu().tolist() == [0, 1, 2, 3, 4, 5, -1, -1] and sts[0].Get_count(MPI.INT) == 6
        return True
    assert H.run_ranks(comms, body) == [True]
    free(comms)


# ---- 7. Probe and Iprobe ---------------------------------------------------------------------------------------------

def test_probe_then_receive_packed_and_unpack():
    comms = world()
    vec = Datatype.Vector(4, 2, 5, MPI.DOUBLE)
    mat = np.arange(20, dtype=np.float64) * 1.5

    def body(c):
        me = c.Rank()
        if me == 1:
            assert c.Iprobe(MPI.ANY_SOURCE, MPI.ANY_TAG) is None and c.Iprobe(0, 7) is None  # nothing before the send
        c.Barrier()
        src = dev(mat)  # alive until the body ends: an eager send returns before its pack has run
        if me == 0:
            c.Send(src, 0, 1, vec, 1, 7)  # eager: it returns with the message unmatched
        c.Barrier()
        if me == 1:
            a = c.Probe(MPI.ANY_SOURCE, MPI.ANY_TAG)
            b = c.Probe(0, 7)  # two probes give the same answer: nothing is consumed
            i = c.Iprobe(0, MPI.ANY_TAG)
            for st in (a, b, i):
                assert (st.source, st.tag, st.Get_count(MPI.DOUBLE), st.Get_count(vec), st.wire_bytes()) == (0, 7, 8, 1, 72)
            assert c.Iprobe(0, 8) is None
            img = torch.zeros(a.wire_bytes(), dtype=torch.uint8, device="cuda")
            st = c.Recv(img, 0, a.wire_bytes(), PACKED, a.source, a.tag)
            assert st.Get_count(PACKED) == 72
            out = dev(np.full(20, -1.0))
            assert c.Unpack(img, 0, out, 0, 1, vec) == 72
            exp = np.full(20, -1.0)
            idx = (np.arange(4)[:, None] * 5 + np.arange(2)[None, :]).reshape(-1)
            exp[idx] = mat[idx]
            same(raw(out), exp, "probe, receive PACKED, unpack")
            assert c.Iprobe(MPI.ANY_SOURCE, MPI.ANY_TAG) is None  # the receive took it
            assert c.Iprobe(MPI.PROC_NULL, 3).source == MPI.PROC_NULL and c.Probe(MPI.PROC_NULL, 3).Get_count(MPI.INT) == 0
        c.Barrier()
        # a PACKED send: the host cannot know its elements; the image it needs is the image sent
        sec = dev(WC.section(5, np.array([5, 6], np.int32)))
        if me == 0:
            c.Send(sec, 0, 16, PACKED, 1, 8)
        else:
            st = c.Probe(0, 8)
            assert st.Get_elements(MPI.INT) == MPI.UNDEFINED and st.wire_bytes() == 16
            got = torch.full((2,), -1, dtype=torch.int32, device="cuda")
            c.Recv(got, 0, 2, MPI.INT, 0, 8)
            assert got.cpu().tolist() == [5, 6]
        with pytest.raises(MPIException) as e:
            c.Iprobe(5, 0)
        assert ERR_ARG in str(e.value)
        with pytest.raises(MPIException) as e:
            c.Probe(0, -7)
        assert ERR_ARG in str(e.value)
        torch.cuda.synchronize()  # an eager send returns before its pack has run: the buffer outlives it
        return True
    assert H.run_ranks(comms, body) == [True, True]
    vec.Free()
    free(comms)


def test_probe_without_a_sender_times_out_on_the_host():
    """A host wait under mpjx_comm_set_p2p_timeout: nothing is enqueued on the GPU; the world is failed afterwards."""
    comms = world()

    def body(c):
        if c.Rank() == 1:
            c.set_p2p_timeout(0.2)
            before = c.p2p_stats()
            with pytest.raises(MPIException) as e:
                c.Probe(0, 1)
            assert ERR_INTERNAL in str(e.value) and "timed out" in str(e.value), str(e.value)
            assert c.p2p_stats() == before
            with pytest.raises(MPIException) as e:
                c.Iprobe(0, 1)
            assert ERR_INTERNAL in str(e.value)
        return True
    assert H.run_ranks(comms, body) == [True, True]
    free(comms)
