"""GPU: the block moves with an irregular datatype (Hvector / Indexed / Hindexed) in-process on device 0:
mpjx_alltoallv_dt at P = 1 (one k_indexed launch), the mirrors' nine methods with an irregular type on either
side in one-device multicore worlds, and the pack -> exchange -> unpack engine under MPJX_SMP_COPY=1. Every
receive buffer starts as a sentinel and is compared whole, byte for byte, against numpy indexing that restates
the reference's rules on its own (tests/indexed_cases.py); send buffers must come back unchanged.

The search takes its LDS form for tables of up to 512 blocks, the most that form can hold (DESIGN.md §4 "Indexed
moves"), and its direct form above: the small cases here run the LDS form, the 1,000- and 5,000-block types the
direct one, and test_both_forms_give_the_same_bytes forces each form on the same cases."""
import ctypes
import os
import threading

import numpy as np
import pytest

import indexed_cases as IC
import strided_cases as SC
from mpjexpress_amd import _lib, mpi
from mpjexpress_amd.mpi import MPI, Datatype, MPIException

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

BASES = ("BYTE", "CHAR", "INT", "DOUBLE", "DOUBLE2")
PLAIN = IC.PLAIN


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


def dt_call(comm, sbuf, sf, st, soff, sc, sd, rbuf, rf, rt, roff, rc, rd, sync=True):
    """mpjx_alltoallv_dt itself on a one-rank world: addresses from the Python offsets (base elements)."""
    i64 = ctypes.c_int64 * 1
    torch.cuda.synchronize()
    _lib.call("mpjx_alltoallv_dt", comm.handle, sbuf.data_ptr() + soff * sf.bsz, i64(sc), i64(sd), st.code,
              rbuf.data_ptr() + roff * rf.bsz, i64(rc), i64(rd), rt.code, None)
    if sync:
        _lib.call("mpjx_comm_synchronize", comm.handle)


def move(one, sf, st, soff, sc, sd, rf, rt, roff, rc, rd, between=None):
    """One P = 1 move of sc items of sf into rc items of rf with library types st, rt; None, or what differs."""
    w = [(SC.Side(sf, soff, [sc], [sd]), SC.Side(rf, roff, [rc], [rd]))]
    send, exp = SC.fill(w)[0]
    sbuf = torch.from_numpy(send).cuda()
    rbuf = torch.full((exp.size,), SC.SENT, dtype=torch.uint8, device="cuda")
    assert sbuf.data_ptr() % 16 == 0 and rbuf.data_ptr() % 16 == 0
    dt_call(one, sbuf, sf, st, soff, sc, sd, rbuf, rf, rt, roff, rc, rd, sync=between is None)
    if between:
        between()
        _lib.call("mpjx_comm_synchronize", one.handle)
    what = f"{sf.base.name} {sf.spec} x{sc} @{soff}+{sd} -> {rf.spec} x{rc} @{roff}+{rd}"
    return SC.differs(rbuf.cpu().numpy(), exp, what) or SC.differs(sbuf.cpu().numpy(), send, what + " (send buffer)")


def p1(one, base, sspec, soff, sc, sd, rspec, roff, rc, rd):
    sf, rf = IC.form(base, sspec), IC.form(base, rspec)
    st, rt = IC.lib_type(sf), IC.lib_type(rf)
    try:
        return move(one, sf, st, soff, sc, sd, rf, rt, roff, rc, rd)
    finally:
        for t in (st, rt):
            t.Free()


def forms(per):
    """The form cases of tests/test_indexed_abi.py; `per` = base elements per item of the base type."""
    f = {"dropped_empty_block": ("I", (3, 1, 0, 2), (7, 0, 4, 12)),
         "lb_4": ("I", (2, 1), (9, 4)),
         "hindexed_back_and_forth": IC.RI,
         "triangle": ("I", tuple(8 - i for i in range(8)), tuple(9 * i for i in range(8))),
         "abutting_merge": ("I", (2, 3, 1), (0, 2, 9)),
         "regular_is_a_vector": ("I", (2, 2, 2), (0, 5, 10)),
         "one_block_lb_3": ("I", (2,), (3,))}
    for off in (0, 1, 2):  # hvec.java: Hvector(3, 1, ext + off, Vector(2, 3, 4, base)), ext = 7 items
        f[f"hvector_of_vector_{off}"] = ("HV", 3, 1, (7 + off) * per, (2, 3, 4))
    return f


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("name", list(forms(1)))
def test_p1_forms_against_a_contiguous_side(one, base, name):
    """Each form as the send type into a contiguous receive and the reverse, with 0, 1 and 3 items (3 pins the
    k * extent stepping, lb not subtracted) and the buffer offset by 0 and 1 element."""
    spec = forms(SC.BASES[base].size)[name]
    size = IC.form(base, spec).size // SC.BASES[base].size
    for items in (0, 1, 3):
        for off in (0, 1):
            assert p1(one, base, spec, off, items, 0, PLAIN, 1 - off, items * size, 2) is None
            assert p1(one, base, PLAIN, 1 - off, items * size, 1, spec, off, items, 0) is None


@pytest.mark.parametrize("base", BASES)
def test_p1_both_sides_irregular(one, base):
    """[3,1,2] into [2,2,2]: different block shapes, displacements that go back and forth, lb = 1 on the
    receive side; 3 items step by each side's own extent."""
    for items in (0, 1, 3):
        for off in (0, 1):
            assert p1(one, base, IC.SI, off, items, 1, IC.RI, 1 - off, items, 3) is None
            assert p1(one, base, IC.RI, off, items, 0, ("V", 3, 2, 5), off, items, 1) is None  # irregular x regular


def permutation(n, unit, seed, ragged=False):
    order = np.random.default_rng(seed).permutation(n)
    return ("I", tuple(int(unit * (1 + i % 3)) if ragged else unit for i in order), tuple(int(4 * unit * i) for i in order))


def test_p1_a_thousand_unit_byte_blocks(one):
    """A permutation of 1,000 one-byte blocks x 3 items: granule 1, 3,000 granules = more than two tiles of
    1,024, and tiles that cross item boundaries; both directions."""
    spec = permutation(1000, 1, 1)
    assert p1(one, "BYTE", spec, 1, 3, 0, PLAIN, 3, 3000, 0) is None
    assert p1(one, "BYTE", PLAIN, 3, 3000, 0, spec, 1, 3, 2) is None


def test_p1_five_thousand_blocks(one):
    """A 5,000-block table: above the LDS form's threshold of 512 blocks (all it can hold), so searched in device
    memory; against a 1,000-block table on the other side."""
    assert p1(one, "INT", permutation(5000, 1, 5), 0, 3, 0, permutation(1000, 5, 6), 1, 3, 0) is None
    assert p1(one, "INT", permutation(5000, 2, 7, ragged=True), 2, 1, 0, PLAIN, 0, 19998, 0) is None


@pytest.mark.parametrize("bl,disp,soff,glog", [((2, 4), (6, 0), 1, 2), ((2, 4), (6, 0), 2, 3), ((4, 8), (12, 0), 4, 4)])
def test_p1_int_blocks_of_granule_4_8_16(one, bl, disp, soff, glog):
    """INT block lengths and offsets that are multiples of 2 (4) elements give granule 8 (16) where the buffer
    offset allows it, 4 one element further (tests/cpp/indexed_plan_test.cpp pins the choice itself)."""
    n = 3 * sum(bl)
    assert n * 4 % (1 << glog) == 0
    assert p1(one, "INT", ("I", bl, disp), soff, 3, 0, PLAIN, soff, n, 0) is None
    assert p1(one, "INT", PLAIN, soff, n, 0, ("I", bl, disp), soff, 3, 0) is None


@pytest.mark.parametrize("cap", [0, 512])
def test_both_forms_give_the_same_bytes(one, cap):
    """MPJX_INDEXED_LDS_MAX_BLOCKS (read per call) sets the largest table searched in LDS: 0 forces the direct
    form, 512 is the default. The same cases under each: a table on both sides, 500 blocks over three tiles,
    and a table larger than LDS can hold beside one it can."""
    old = os.environ.get("MPJX_INDEXED_LDS_MAX_BLOCKS")
    os.environ["MPJX_INDEXED_LDS_MAX_BLOCKS"] = str(cap)
    try:
        for base in ("BYTE", "DOUBLE2"):
            assert p1(one, base, IC.SI, 1, 3, 1, IC.RI, 0, 3, 3) is None
        assert p1(one, "BYTE", permutation(500, 1, 1), 1, 5, 0, PLAIN, 3, 2500, 0) is None
        assert p1(one, "INT", permutation(5000, 1, 5), 0, 3, 0, permutation(500, 10, 6), 1, 3, 0) is None
    finally:
        if old is None:
            del os.environ["MPJX_INDEXED_LDS_MAX_BLOCKS"]
        else:
            os.environ["MPJX_INDEXED_LDS_MAX_BLOCKS"] = old


def test_p1_streaming_form_at_64_mib(one):
    """64 MiB packed in one call: the non-temporal form (512 lanes x 1 granule). 16 items of a permutation of
    4,096 blocks of 1 KiB, 2 KiB apart, into a contiguous buffer."""
    nb, bl = 4096, 256  # ints
    order = np.random.default_rng(3).permutation(nb)
    row = Datatype.Contiguous(bl, MPI.INT)
    t = Datatype.Indexed([1] * nb, [int(2 * i) for i in order], row)
    row.Free()
    try:
        assert (t.Size(), t.Extent()) == (nb * bl, (2 * nb - 1) * bl)
        items = 16
        src = torch.arange(items * t.Extent() + bl, dtype=torch.int32, device="cuda")
        dst = torch.full((items * t.Size() + 8,), -1, dtype=torch.int32, device="cuda")
        one.Alltoall(src, 0, items, t, dst, 4, items * t.Size(), MPI.INT)
        torch.cuda.synchronize()
        idx = torch.from_numpy(order.astype(np.int64) * 2 * bl).cuda()
        want = (torch.arange(items, device="cuda")[:, None, None] * t.Extent() + idx[None, :, None]
                + torch.arange(bl, device="cuda")[None, None, :]).reshape(-1).to(torch.int32)
        assert torch.equal(dst[4:-4], want)
        assert bool((dst[:4] == -1).all()) and bool((dst[-4:] == -1).all())
    finally:
        t.Free()


# ---- worlds -----------------------------------------------------------------------------------------------
def methods(comms, base="INT"):
    P = len(comms)
    todo = IC.matrix(P)

    def body(c):
        types = {}
        try:
            return IC.run_methods(torch, c, P, base, todo, types)
        finally:
            for t in types.values():
                t.Free()
    out, err = run_ranks(comms, body)
    assert not any(err), err
    bad = [m for r in out for m in r]
    assert not bad, bad[:6]
    return len(todo)


@pytest.mark.parametrize("P", [2, 3])
def test_nine_methods_with_an_irregular_type_on_either_side(P):
    """All nine mirror methods, an irregular type on the send side, on the receive side and on both (of
    different blocking); rooted calls at roots 0 and P - 1; ragged counts, displacements with gaps."""
    comms = world(P)
    try:
        assert methods(comms) == 3 * (4 + 2 * 5)
        assert methods(comms, "DOUBLE2") == 3 * (4 + 2 * 5)
    finally:
        free(comms)


def test_smp_exchange_engine():
    """MPJX_SMP_COPY=1 (read per call) at P = 3: irregular sends packed into scratch, SmpTransport::exchange,
    irregular receives unpacked; the rank's own block from layout to layout."""
    old = os.environ.get("MPJX_SMP_COPY")
    os.environ["MPJX_SMP_COPY"] = "1"
    comms = world(3)
    try:
        assert methods(comms) == 3 * (4 + 2 * 5)
        assert methods(comms, "BYTE") == 3 * (4 + 2 * 5)
    finally:
        free(comms)
        if old is None:
            del os.environ["MPJX_SMP_COPY"]
        else:
            os.environ["MPJX_SMP_COPY"] = old


def test_more_segments_than_one_table():
    """Alltoall at P = 9 with irregular types on both sides is 81 indexed segments: four launches of rank 0 on
    one stream (24 segments per table)."""
    P = 9
    comms = world(P)
    try:
        w = IC.method_world("alltoall", P, "INT", "both")
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


# ---- errors and ordering ------------------------------------------------------------------------------------
def test_self_overlapping_type_sends_but_does_not_receive():
    """hvec.java with big_offset = -1: Hvector(3, 1, 6, Vector(2, 3, 4, INT)) reads element 6 (and 12) twice.
    Legal to send; as a receive type MPJX_ERR_ARG with the receive buffer untouched."""
    spec = ("HV", 3, 1, 6, (2, 3, 4))
    comms = world(1)
    try:
        for items in (1, 3):
            assert p1(comms[0], "INT", spec, 1, items, 0, PLAIN, 0, 18 * items, 1) is None
    finally:
        free(comms)
    comms = world(1)  # the rejected call leaves its world failed
    t = IC.form("INT", spec).make()
    try:
        s = torch.arange(64, dtype=torch.int32, device="cuda")
        r = torch.full((64,), -1, dtype=torch.int32, device="cuda")
        with pytest.raises(MPIException, match=r"\(-1\).*share a byte"):
            comms[0].Alltoallv(s, 0, [18], [0], MPI.INT, r, 0, [1], [0], t)
        torch.cuda.synchronize()
        assert bool((r == -1).all()), "the rejected call wrote"
    finally:
        t.Free()
        free(comms)


def test_two_irregular_receive_layouts():
    """Rank 1 receives one item of Indexed([1,1],[0,4]) (elements 0 and 4) from each rank: at displacements 0
    and 1 the layouts interleave and share nothing (accepted); at 0 and 4 they share element 4 and the world
    fails on every rank."""
    for disp, ok in (([0, 1], True), ([0, 4], False)):
        comms = world(2)

        def body(c):
            t = Datatype.Indexed([1, 1], [0, 4], MPI.INT)
            s = torch.arange(16, dtype=torch.int32, device="cuda") + 100 * c.Rank()
            r = torch.full((16,), -1, dtype=torch.int32, device="cuda")
            try:
                c.Alltoallv(s, 0, [2, 2], [0, 2], MPI.INT, r, 0, [1, 1], disp if c.Rank() == 1 else [0, 2], t)
                return r.cpu().tolist()
            finally:
                t.Free()
        try:
            out, err = run_ranks(comms, body, limit=30)
            if ok:
                assert not any(err), err
                assert out[1][:6] == [2, 102, -1, -1, 3, 103] and set(out[1][6:]) == {-1}, out[1]
                assert out[0][:8] == [0, -1, 100, -1, 1, -1, 101, -1], out[0]
            else:
                assert all(isinstance(e, MPIException) for e in err), err
                assert "overlap" in str(err[1]) and "(-1)" in str(err[1]), err[1]
        finally:
            free(comms)


def test_type_freed_between_enqueue_and_synchronise(one):
    """MPI's Type_free promise: the enqueued call completes with the layout it was given. The first use of each
    type here also uploads its table on the call's stream, after which the code is released at once."""
    sf, rf = IC.form("INT", permutation(702, 3, 11, ragged=True)), IC.form("INT", IC.RI)
    st, rt = sf.make(), rf.make()
    n = sf.size // 6
    assert sf.size % 6 == 0
    assert move(one, sf, st, 1, 1, 0, rf, rt, 0, n, 2, between=lambda: (st.Free(), rt.Free())) is None
    with pytest.raises(_lib.MPJXError, match=r"\(-1\).*unknown or freed"):
        _lib.call("mpjx_type_info", st.code, None, None, None)
