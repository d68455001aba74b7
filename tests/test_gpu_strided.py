"""GPU: the strided block moves in-process on device 0: mpjx_alltoallv_dt at P = 1 (one k_strided launch), the
mirrors' nine methods with a Vector on either side in one-device multicore worlds (one launch by rank 0 for the
whole world), and the pack -> exchange -> unpack engine under MPJX_SMP_COPY=1. Every receive buffer starts
as a sentinel and is compared whole, byte for byte, against numpy indexing (tests/strided_cases.py): a write
into a gap between two blocks fails like a wrong byte; send buffers must come back unchanged."""
import ctypes
import os
import threading

import numpy as np
import pytest

import strided_cases as SC
from mpjexpress_amd import _lib, mpi
from mpjexpress_amd.mpi import MPI, Datatype, MPIException

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


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


def world(P):
    return mpi.smp_world(P, [0] * P)


def free(comms):
    for c in comms:
        c.Free()


@pytest.fixture(scope="module")
def one():
    comms = world(1)
    yield comms[0]
    free(comms)


def dt_call(comm, sbuf, sform, stype, soff, sc, sd, rbuf, rform, rtype, roff, rc, rd):
    """mpjx_alltoallv_dt itself on a one-rank world: addresses from the Python offsets (base elements)."""
    i64 = ctypes.c_int64 * 1
    torch.cuda.synchronize()
    _lib.call("mpjx_alltoallv_dt", comm.handle, sbuf.data_ptr() + soff * sform.bsz, i64(sc), i64(sd), stype.code,
              rbuf.data_ptr() + roff * rform.bsz, i64(rc), i64(rd), rtype.code, None)
    _lib.call("mpjx_comm_synchronize", comm.handle)


def p1(one, base, sspec, soff, sc, sd, rspec, roff, rc, rd):
    """One P = 1 move of sc items of sspec into rc items of rspec; None, or what differs."""
    sf, rf = SC.Form(base, sspec), SC.Form(base, rspec)
    w = [(SC.Side(sf, soff, [sc], [sd]), SC.Side(rf, roff, [rc], [rd]))]
    send, exp = SC.fill(w)[0]
    st = sf.base if sspec == ("C", 1) else sf.make()
    rt = rf.base if rspec == ("C", 1) else rf.make()
    try:
        sbuf = torch.from_numpy(send).cuda()
        rbuf = torch.full((exp.size,), SC.SENT, dtype=torch.uint8, device="cuda")
        assert sbuf.data_ptr() % 16 == 0 and rbuf.data_ptr() % 16 == 0
        dt_call(one, sbuf, sf, st, soff, sc, sd, rbuf, rf, rt, roff, rc, rd)
        what = f"{base} {sspec} x{sc} @{soff}+{sd} -> {rspec} x{rc} @{roff}+{rd}"
        return SC.differs(rbuf.cpu().numpy(), exp, what) or SC.differs(sbuf.cpu().numpy(), send, what + " (send buffer)")
    finally:
        for t in (st, rt):
            t.Free()


PLAIN = ("C", 1)
P1_CASES = {
    # granule 1: bytes at odd addresses on both sides
    "byte_vector_to_contiguous": ("BYTE", ("V", 5, 3, 7), 3, 2, 0, PLAIN, 1, 30, 0),
    # granule 2
    "char_vector": ("CHAR", ("V", 4, 3, 5), 1, 3, 0, ("V", 4, 3, 5), 1, 3, 2),
    # granule 4: different blocking on the two sides, items step by the extent
    "int_vector_to_other_vector": ("INT", ("V", 6, 2, 5), 1, 3, 0, ("V", 4, 3, 7), 1, 3, 1),
    # granule 8: a column of a 33 x 17 matrix into a row, and back
    "double_column_to_contiguous": ("DOUBLE", ("V", 33, 1, 17), 0, 1, 3, PLAIN, 1, 33, 0),
    "double_contiguous_to_column": ("DOUBLE", PLAIN, 1, 33, 0, ("V", 33, 1, 17), 0, 1, 5),
    # granule 16 at a 16-B-aligned base, 8 one element further
    "double_blocks_aligned": ("DOUBLE", ("V", 9, 4, 10), 0, 2, 0, ("V", 9, 4, 10), 0, 2, 2),
    "double_blocks_plus_one": ("DOUBLE", ("V", 9, 4, 10), 1, 2, 0, ("V", 9, 4, 10), 1, 2, 2),
    # stride in pairs
    "double2_vector": ("DOUBLE2", ("V", 3, 2, 4), 2, 2, 0, ("C", 4), 0, 3, 2),
    # more than one tile (1024 granules) and a last tile that is not full
    "int_two_tiles_and_a_bit": ("INT", ("V", 6, 2, 5), 1, 200, 0, ("V", 4, 3, 7), 3, 200, 1),
    # nothing to move
    "empty_type": ("INT", ("V", 0, 3, 7), 1, 5, 0, PLAIN, 1, 0, 0),
    "zero_blocklength": ("INT", ("V", 4, 0, 7), 1, 5, 0, ("V", 0, 1, 2), 1, 9, 0),
    "zero_counts": ("INT", ("V", 6, 2, 5), 1, 0, 0, ("V", 4, 3, 7), 1, 0, 0),
}


@pytest.mark.parametrize("name", list(P1_CASES))
def test_p1_smallest_shapes(one, name):
    assert p1(one, *P1_CASES[name]) is None


def test_two_contiguous_types_equal_alltoallv(one):
    """Contiguous(3, INT) x 5 into INT x 15 at odd offsets: the block-move kernel, byte for byte what
    mpjx_alltoallv stores for the same bytes."""
    i64 = ctypes.c_int64 * 1
    send = np.random.default_rng(5).integers(0, 256, 256, dtype=np.uint8)
    sbuf = torch.from_numpy(send).cuda()
    c3 = Datatype.Contiguous(3, MPI.INT)
    got = []
    try:
        for which in ("dt", "plain"):
            rbuf = torch.full((256,), SC.SENT, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            if which == "dt":  # displacements in base elements on both sides
                _lib.call("mpjx_alltoallv_dt", one.handle, sbuf.data_ptr() + 4, i64(5), i64(2), c3.code,
                          rbuf.data_ptr() + 8, i64(15), i64(3), MPI.INT.code, None)
            else:
                _lib.call("mpjx_alltoallv", one.handle, sbuf.data_ptr() + 4, i64(15), i64(2), rbuf.data_ptr() + 8, i64(15),
                          i64(3), MPI.INT.code, None)
            _lib.call("mpjx_comm_synchronize", one.handle)
            got.append(rbuf.cpu().numpy())
    finally:
        c3.Free()
    exp = np.full(256, SC.SENT, np.uint8)
    exp[20:80] = send[12:72]
    assert np.array_equal(got[1], exp)
    assert np.array_equal(got[0], got[1])


def methods(comms, base="INT"):
    P = len(comms)
    todo = SC.matrix(P)

    def body(c):
        types = {}
        try:
            return SC.run_methods(torch, c, P, base, todo, types)
        finally:
            for t in types.values():
                t.Free()
    out, err = run_ranks(comms, body)
    assert not any(err), err
    bad = [m for r in out for m in r]
    assert not bad, bad[:6]
    return len(todo)


@pytest.mark.parametrize("P", [2, 3])
def test_nine_methods_with_a_vector_on_either_side(P):
    """All nine mirror methods, a Vector on the send side, on the receive side and on both (of different
    blocking); rooted calls at roots 0 and P - 1; ragged counts, displacements with gaps in base elements."""
    comms = world(P)
    try:
        assert methods(comms) == 3 * (4 + 2 * 5)
    finally:
        free(comms)


def test_smp_exchange_engine():
    """MPJX_SMP_COPY=1 (read per call) at P = 3: pack -> SmpTransport::exchange -> unpack, the rank's own
    block from layout to layout."""
    old = os.environ.get("MPJX_SMP_COPY")
    os.environ["MPJX_SMP_COPY"] = "1"
    comms = world(3)
    try:
        assert methods(comms) == 3 * (4 + 2 * 5)
        assert methods(comms, "DOUBLE2") == 3 * (4 + 2 * 5)
    finally:
        free(comms)
        if old is None:
            del os.environ["MPJX_SMP_COPY"]
        else:
            os.environ["MPJX_SMP_COPY"] = old


def test_transpose_by_alltoallv_at_p4():
    """A (4 * 8) x (4 * 8) DOUBLE matrix distributed by rows, 8 per rank. A column of a rank's 8 x 32 panel is
    Vector(8, 1, 32); displacements are base elements, so column 8 j + k is that type at displacement 8 j + k
    with no resized type. Call k of 8 sends rank j column k of its block and stores what rank i sent as 8
    plain doubles at 64 i + 8 k: row k of block i of the transposed panel. numpy.transpose gives the whole."""
    P, B = 4, 8
    N = P * B
    A = np.random.default_rng(11).standard_normal((N, N))
    comms = world(P)

    def body(c):
        me = c.Rank()
        col = Datatype.Vector(B, 1, N, MPI.DOUBLE)
        s = torch.from_numpy(A[me * B:(me + 1) * B].copy()).cuda().view(-1)
        r = torch.full((B * N,), float("nan"), dtype=torch.float64, device="cuda")
        try:
            for k in range(B):
                c.Alltoallv(s, 0, [1] * P, [B * j + k for j in range(P)], col, r, 0, [B] * P,
                            [B * B * i + B * k for i in range(P)], MPI.DOUBLE)
        finally:
            col.Free()
        return r.cpu().numpy()
    try:
        out, err = run_ranks(comms, body)
        assert not any(err), err
    finally:
        free(comms)
    T = np.transpose(A)
    for me in range(P):
        # rank me holds rows 8 me .. 8 me + 7 of T, block i (its columns 8 i .. 8 i + 7) row-major at 64 i
        got = out[me].reshape(P, B, B)
        for i in range(P):
            assert np.array_equal(got[i], T[me * B:(me + 1) * B, i * B:(i + 1) * B]), (me, i)


def test_more_segments_than_one_table():
    """Alltoall at P = 9 with a Vector send type is 81 strided segments: three launches of rank 0 on one stream
    (32 segments per table)."""
    P = 9
    comms = world(P)
    try:
        w = SC.method_world("alltoall", P, "INT", "both")
        data = SC.fill(w, seed=9)

        def body(c):
            me = c.Rank()
            s, q = w[me]
            st, rt = s.form.make(), q.form.make()
            try:
                sbuf = torch.from_numpy(data[me][0]).cuda().view(torch.int32)
                rbuf = torch.full((data[me][1].size,), SC.SENT, dtype=torch.uint8, device="cuda").view(torch.int32)
                SC.method_call(c, "alltoall", s, q, st, rt, sbuf, rbuf, 0)
                return SC.differs(rbuf.view(torch.uint8).cpu().numpy(), data[me][1], f"rank {me}")
            finally:
                st.Free()
                rt.Free()
        out, err = run_ranks(comms, body)
        assert not any(err), err
        assert not any(out), out
    finally:
        free(comms)


# ---- errors ---------------------------------------------------------------------------------------------
def test_packed_length_mismatch_raises_on_every_rank_and_moves_nothing():
    comms = world(2)

    def body(c):
        v = Datatype.Vector(3, 2, 5, MPI.INT)  # 6 elements
        s = torch.arange(256, dtype=torch.int32, device="cuda")
        r = torch.full((256,), -1, dtype=torch.int32, device="cuda")
        # every rank sends rank 0 one item and rank 1 two (48 bytes); rank 1 expects 11 ints (44 bytes) from rank 0
        rc = [11, 12] if c.Rank() == 1 else [6, 6]
        try:
            c.Alltoallv(s, 0, [1, 2], [0, 40], v, r, 0, rc, [0, 100], MPI.INT)
        except MPIException as e:
            torch.cuda.synchronize()
            return str(e), bool((r == -1).all())
        finally:
            v.Free()
        return None, False
    try:
        out, err = run_ranks(comms, body, limit=30)
        assert not any(err), err
        for msg, untouched in out:
            assert msg and "rank 0 sends 48 bytes to rank 1, which receives 44" in msg and "(-1)" in msg, out
            assert untouched, "a receive buffer was written"
    finally:
        free(comms)


def test_the_same_column_received_twice_fails_the_world():
    """Rank 1 receives two columns of one matrix from ranks 0 and 1: interleaved ones are the legitimate gather
    pattern (first world); the same column twice is an overlap (second world), and fails every rank."""
    for cols, ok in (([0, 1, 2], True), ([2, 1, 2], False)):
        comms = world(3)

        def body(c):
            col = Datatype.Vector(4, 1, 3, MPI.INT)  # a column of a 4 x 3 matrix
            s = torch.arange(64, dtype=torch.int32, device="cuda") + 100 * c.Rank()
            r = torch.full((64,), -1, dtype=torch.int32, device="cuda")
            try:
                c.Alltoallv(s, 0, [4, 4, 4], [0, 8, 16], MPI.INT, r, 0, [1, 1, 1],
                            cols if c.Rank() == 1 else [0, 1, 2], col)
                return r[:12].cpu().numpy().reshape(4, 3)
            finally:
                col.Free()
        try:
            out, err = run_ranks(comms, body, limit=30)
            if ok:
                assert not any(err), err
                for me in range(3):
                    for i in range(3):
                        assert out[me][:, i].tolist() == [100 * i + 8 * me + k for k in range(4)], (me, i, out[me])
            else:
                assert all(isinstance(e, MPIException) for e in err), err
                assert "overlap" in str(err[1]) and "(-1)" in str(err[1]), err[1]
        finally:
            free(comms)


def test_mirror_argument_errors(one):
    s = torch.zeros(64, dtype=torch.int32, device="cuda")
    r = torch.zeros(64, dtype=torch.int32, device="cuda")
    v = Datatype.Vector(3, 2, 5, MPI.INT)
    try:
        with pytest.raises(MPIException, match="base type"):
            one.Alltoallv(s, 0, [1], [0], v, r.view(torch.float32), 0, [6], [0], MPI.FLOAT)
        with pytest.raises(MPIException, match="span"):  # 6 items span 72 elements
            one.Alltoallv(s, 0, [6], [0], v, r, 0, [36], [0], MPI.INT)
        with pytest.raises(MPIException, match="differ in length"):
            one.Alltoall(s, 0, 1, v, r, 0, 5, MPI.INT)
        assert v.Size() == 6 and v.Extent() == 12 and v.Lb() == 0 and v.Ub() == 12
        v.Commit()
    finally:
        v.Free()
    comms = world(1)  # the rejected call leaves its world failed
    try:
        with pytest.raises(MPIException, match=r"\(-1\)"):  # use after free, rejected by the library
            comms[0].Alltoallv(s, 0, [1], [0], v, r, 0, [6], [0], MPI.INT)
    finally:
        free(comms)


def test_existing_alltoallv_still_rejects_a_derived_code():
    """mpjx_type_size() is 0 for a derived code, so mpjx_alltoallv answers it as it answers any unknown type."""
    s = torch.zeros(64, dtype=torch.int32, device="cuda")
    r = torch.zeros(64, dtype=torch.int32, device="cuda")
    v = Datatype.Vector(3, 2, 5, MPI.INT)
    comms = world(1)
    one64 = (ctypes.c_int64 * 1)
    try:
        with pytest.raises(_lib.MPJXError, match=r"\(-1\).*unknown datatype code") as e:
            _lib.call("mpjx_alltoallv", comms[0].handle, s.data_ptr(), one64(1), one64(0), r.data_ptr(), one64(1), one64(0),
                      v.code, None)
        assert e.value.status == -1
        torch.cuda.synchronize()
        assert not r.any(), "the rejected call wrote"
    finally:
        free(comms)
        v.Free()
