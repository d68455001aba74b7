"""GPU: k_transpose, the element transpose among the strided moves, in-process on device 0.

A column of a row-major matrix resized to one element (Struct with an UB marker) makes `C` items `C` adjacent
columns; moving them into a contiguous run (gather) or back (scatter) is the transpose of an R x C panel. For
granules of 1, 2, 4, 8 and 16 bytes (BYTE, SHORT, INT, DOUBLE, DOUBLE2) and R, C in {2, T-1, T, T+1, 2T+1} with T
the kernel's tile side, the panel sits inside a wider matrix at a nonzero offset, the whole receive buffer
starts as a sentinel and is compared byte for byte with numpy's a[:R, :C].T; mpjx_comm_last_move_kernels must
say k_transpose, and the same call under MPJX_TRANSPOSE=0 must store the same bytes through k_strided. Near
misses keep k_strided, a world of 6 rank threads fills more than one launch table, and none of the existing
strided cases reaches the new kernel.
"""
import ctypes
import os

import numpy as np
import pytest

import strided_cases as SC
from mpjexpress_amd import _lib
from mpjexpress_amd.mpi import MPI, Datatype
from test_gpu_strided import free, run_ranks, world

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K_MOVES, K_STRIDED, K_INDEXED, K_TRANSPOSE = 1, 2, 4, 8
SENT = 0xA5
# name -> (type, base elements per element, bytes per base element, tile side)
GRANULES = {"BYTE": (MPI.BYTE, 1, 1, 64), "SHORT": (MPI.SHORT, 1, 2, 64), "INT": (MPI.INT, 1, 4, 64),
            "DOUBLE": (MPI.DOUBLE, 1, 8, 32), "DOUBLE2": (MPI.DOUBLE2, 2, 8, 32)}


@pytest.fixture(scope="module")
def one():
    comms = world(1)
    yield comms[0]
    free(comms)


@pytest.fixture(autouse=True)
def knob():
    old = os.environ.pop("MPJX_TRANSPOSE", None)
    yield
    os.environ.pop("MPJX_TRANSPOSE", None)
    if old is not None:
        os.environ["MPJX_TRANSPOSE"] = old


def kernels(comm):
    m = ctypes.c_uint(99)
    _lib.call("mpjx_comm_last_move_kernels", comm.handle, ctypes.byref(m))
    return m.value


def column(R, ld, old, ub=None):
    """Vector(R, 1, ld, old) with an UB marker `ub` base elements in (default: one element of old)."""
    v = Datatype.Vector(R, 1, ld, old)
    t = Datatype.Struct([1, 1], [0, old.size if ub is None else ub], [v, MPI.UB])
    v.Free()
    return t


def move(comm, sbuf, soff, sc, st, rbuf, roff, rc, rt, bsz):
    """mpjx_alltoallv_dt on a one-rank world; offsets in base elements. Returns the kernel mask."""
    i64 = ctypes.c_int64 * 1
    torch.cuda.synchronize()
    _lib.call("mpjx_alltoallv_dt", comm.handle, sbuf.data_ptr() + soff * bsz, i64(sc), i64(0), st.code,
              rbuf.data_ptr() + roff * bsz, i64(rc), i64(0), rt.code, None)
    _lib.call("mpjx_comm_synchronize", comm.handle)
    return kernels(comm)


def both_ways(comm, send, soff, sc, st, exp, roff, rc, rt, bsz, want, what):
    """The call with the kernel `want`, then under MPJX_TRANSPOSE=0 through k_strided: the whole receive buffer
    equals `exp` both times and the send buffer is unchanged."""
    sbuf = torch.from_numpy(send).cuda()
    for knob_off in (False, True):
        if knob_off:
            os.environ["MPJX_TRANSPOSE"] = "0"
        else:
            os.environ.pop("MPJX_TRANSPOSE", None)
        rbuf = torch.full((exp.size,), SENT, dtype=torch.uint8, device="cuda")
        mask = move(comm, sbuf, soff, sc, st, rbuf, roff, rc, rt, bsz)
        assert mask == (K_STRIDED if knob_off else want), (what, knob_off, mask)
        bad = SC.differs(rbuf.cpu().numpy(), exp, f"{what} MPJX_TRANSPOSE={'0' if knob_off else 'unset'}")
        assert bad is None, bad
    os.environ.pop("MPJX_TRANSPOSE", None)
    assert np.array_equal(sbuf.cpu().numpy(), send), what


def panel_case(comm, name, R, C, gather, seed):
    old, per, bsz, _ = GRANULES[name]
    esz = per * bsz
    ld, rows, c0, off = C + 3, R + 1, 2, 1  # the panel: rows 0..R of columns c0..c0+C, `off` elements into the buffer
    rng = np.random.default_rng(seed)
    E = np.dtype((np.void, esz))
    col = column(R, ld, old)
    try:
        assert (col.Size(), col.Extent()) == (R * per, per)
        nmat, nrun = (off + rows * ld) * esz + 16, (off + R * C) * esz + 16
        if gather:
            send = rng.integers(0, 256, nmat, dtype=np.uint8)
            a = send[off * esz:(off + rows * ld) * esz].view(E).reshape(rows, ld)
            exp = np.full(nrun, SENT, np.uint8)
            exp[off * esz:(off + R * C) * esz].view(E)[:] = a[:R, c0:c0 + C].T.ravel()
            both_ways(comm, send, (off + c0) * per, C, col, exp, off * per, R * C, old, bsz, K_TRANSPOSE,
                      f"{name} gather {R}x{C}")
        else:
            send = rng.integers(0, 256, nrun, dtype=np.uint8)
            src = send[off * esz:(off + R * C) * esz].view(E).reshape(C, R)
            exp = np.full(nmat, SENT, np.uint8)
            a = exp[off * esz:(off + rows * ld) * esz].view(E).reshape(rows, ld)
            a[:R, c0:c0 + C] = src.T
            both_ways(comm, send, off * per, R * C, old, exp, (off + c0) * per, C, col, bsz, K_TRANSPOSE,
                      f"{name} scatter {R}x{C}")
    finally:
        col.Free()


@pytest.mark.parametrize("gather", (True, False), ids=("gather", "scatter"))
@pytest.mark.parametrize("name", list(GRANULES))
def test_every_granule_and_tile_edge(one, name, gather):
    T = GRANULES[name][3]
    dims = (2, T - 1, T, T + 1, 2 * T + 1)
    n = 0
    for R in dims:
        for C in dims:
            panel_case(one, name, R, C, gather, seed=1000 * R + C)
            n += 1
    assert n == 25


def regular_index(count, first, nblocks, blocklen, stride, extent):
    k = np.arange(count, dtype=np.int64)[:, None, None] * extent
    b = np.arange(nblocks, dtype=np.int64)[None, :, None] * stride
    w = np.arange(blocklen, dtype=np.int64)[None, None, :]
    return (first + k + b + w).ravel()


def near_miss(comm, st, sidx, rt, ridx, what, want=K_STRIDED):
    """INT elements: packed element i of the send layout (index sidx[i]) lands at index ridx[i]."""
    n = int(max(sidx.max(), ridx.max())) + 5
    send = np.random.default_rng(len(what)).integers(0, 256, 4 * n, dtype=np.uint8)
    exp = np.full(4 * n, SENT, np.uint8)
    exp.view(np.uint32)[ridx] = send.view(np.uint32)[sidx]
    sbuf = torch.from_numpy(send).cuda()
    rbuf = torch.full((exp.size,), SENT, dtype=torch.uint8, device="cuda")
    # a regular layout's first packed element is its origin
    mask = move(comm, sbuf, int(sidx[0]), st[1], st[0], rbuf, int(ridx[0]), rt[1], rt[0], 4)
    assert mask == want, (what, mask)
    bad = SC.differs(rbuf.cpu().numpy(), exp, what)
    assert bad is None, bad


def test_near_misses_keep_k_strided(one):
    R, C, ld = 9, 7, 11  # an odd row stride keeps the granule at one INT
    made = []
    try:
        # a block of two granules, resized to two elements
        v2 = Datatype.Vector(R, 2, ld, MPI.INT)
        two = Datatype.Struct([1, 1], [0, 2], [v2, MPI.UB])
        made += [v2, two]
        idx = regular_index(4, 1, R, 2, ld, 2)
        near_miss(one, (two, 4), idx, (MPI.INT, idx.size), np.arange(idx.size) + 3, "two granules per block, gather")
        near_miss(one, (MPI.INT, idx.size), np.arange(idx.size) + 3, (two, 4), idx, "two granules per block, scatter")
        # eb != bb: every other column
        wide = column(R, ld, MPI.INT, ub=2)
        made.append(wide)
        idx = regular_index(5, 1, R, 1, ld, 2)
        near_miss(one, (wide, 5), idx, (MPI.INT, idx.size), np.arange(idx.size) + 2, "extent of two elements, gather")
        near_miss(one, (MPI.INT, idx.size), np.arange(idx.size) + 2, (wide, 5), idx, "extent of two elements, scatter")
        # both sides strided: an R x C panel into the C x R panel of another matrix, column by column
        a, b = column(R, ld, MPI.INT), column(C, ld + 2, MPI.INT)
        made += [a, b]
        near_miss(one, (a, C), regular_index(C, 1, R, 1, ld, 1), (b, R), regular_index(R, 2, C, 1, ld + 2, 1),
                  "both sides strided")
        # one column (a plain Vector: one item) and one row are not transposes either
        v = Datatype.Vector(R, 1, ld, MPI.INT)
        made.append(v)
        near_miss(one, (v, 1), regular_index(1, 1, R, 1, ld, R * ld), (MPI.INT, R), np.arange(R) + 1, "one item")
        # and the transpose itself, for contrast
        near_miss(one, (a, C), regular_index(C, 1, R, 1, ld, 1), (MPI.INT, R * C), np.arange(R * C) + 1,
                  "the column panel", want=K_TRANSPOSE)
    finally:
        for t in made:
            t.Free()


def test_a_misaligned_base_lowers_the_granule_and_keeps_k_strided(one):
    """DOUBLE columns whose matrix starts 4 bytes off an 8-byte boundary cannot be moved in 8-byte granules."""
    R, C, ld = 5, 6, 9
    col = column(R, ld, MPI.DOUBLE)
    try:
        send = np.random.default_rng(3).integers(0, 256, 8 * (R * ld + 4), dtype=np.uint8)
        sbuf = torch.from_numpy(send).cuda()
        rbuf = torch.full((8 * (R * C + 2),), SENT, dtype=torch.uint8, device="cuda")
        i64 = ctypes.c_int64 * 1
        torch.cuda.synchronize()
        _lib.call("mpjx_alltoallv_dt", one.handle, sbuf.data_ptr() + 4, i64(C), i64(0), col.code,
                  rbuf.data_ptr() + 8, i64(R * C), i64(0), MPI.DOUBLE.code, None)
        _lib.call("mpjx_comm_synchronize", one.handle)
        assert kernels(one) == K_STRIDED
        a = send[4:4 + 8 * R * ld].view(np.uint64).reshape(R, ld)
        exp = np.full(rbuf.numel(), SENT, np.uint8)
        exp[8:8 + 8 * R * C].view(np.uint64)[:] = a[:, :C].T.ravel()
        assert SC.differs(rbuf.cpu().numpy(), exp, "misaligned double columns") is None
    finally:
        col.Free()


def test_more_segments_than_one_table_holds():
    """Alltoall of column panels among 6 rank threads on one device: rank 0 launches the world's 36 transposes,
    which is more than the 32 segments of one launch table."""
    P, R, k = 6, 37, 5  # rank i's matrix is R x (P * k): k columns to every rank
    ld = P * k + 1
    mats = [np.random.default_rng(50 + i).integers(0, 1 << 62, (R, ld), dtype=np.int64) for i in range(P)]
    comms = world(P)

    def body(c):
        me = c.Rank()
        col = column(R, ld, MPI.LONG)
        try:
            s = torch.from_numpy(mats[me]).cuda().reshape(-1)
            r = torch.full((P * R * k + 3,), -1, dtype=torch.int64, device="cuda")
            c.Alltoall(s, 0, k, col, r, 1, R * k, MPI.LONG)
            torch.cuda.synchronize()
            return r.cpu().numpy(), kernels(c)
        finally:
            col.Free()
    try:
        out, err = run_ranks(comms, body)
    finally:
        free(comms)
    assert not any(err), err
    for me in range(P):
        got, mask = out[me]
        exp = np.full(P * R * k + 3, -1, np.int64)
        for i in range(P):  # from rank i: its columns me*k .. me*k+k, column by column
            exp[1 + i * R * k:1 + (i + 1) * R * k] = mats[i][:, me * k:(me + 1) * k].T.ravel()
        assert np.array_equal(got, exp), me
        assert mask == (K_TRANSPOSE if me == 0 else 0), (me, mask)


@pytest.mark.parametrize("P", (1, 3))
def test_the_existing_strided_shapes_never_reach_the_new_kernel(P):
    """Every (method, mode, root) of tests/strided_cases.py, rerun: byte-exact as before, and k_transpose in no mask."""
    comms = world(P)
    todo = SC.matrix(P)

    def body(c):
        types, bad, masks = {}, [], []
        try:
            for item in todo:
                bad += SC.run_methods(torch, c, P, "INT", [item], types)
                masks.append(kernels(c))
        finally:
            for t in types.values():
                t.Free()
        return bad, masks
    try:
        out, err = run_ranks(comms, body, limit=120)
    finally:
        free(comms)
    assert not any(err), err
    seen = 0
    for bad, masks in out:
        assert not bad, bad[:3]
        assert len(masks) == len(todo) and not any(m & K_TRANSPOSE for m in masks), masks
        seen |= int(np.bitwise_or.reduce(masks))
    assert seen & K_STRIDED  # the Vectors did run, on the kernel they always ran on
