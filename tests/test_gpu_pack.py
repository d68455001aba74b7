"""GPU: mpjx_pack / mpjx_unpack / mpjx_pack_size on device 0 (k_pack: layout, byte swap and section header in
one pass), through the C ABI and the Python mirror.

Expected images are built here with numpy, independently of the library: the layout's element index from
tests/strided_cases.py / tests/indexed_cases.py (Form / IForm.index(count, first)), `.astype('>u…')` for the
payload, the 8 header bytes written by hand. Whole buffers are compared byte for byte: the image including a
sentinel fill around the section, and the unpack target including the gaps between the type's blocks. Elements
are seeded random bit patterns moved as unsigned integers of the base word's width, so every byte lane counts.

No test provokes a fault: the malformed images are rejected by the kernel's header check before any payload load.
"""
import ctypes
import struct

import numpy as np
import pytest

import indexed_cases as IC
import oracle as O
import strided_cases as SC
from mpjexpress_amd import _lib, mpi
from mpjexpress_amd.mpi import MPI, Datatype, MPIException

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SENT = SC.SENT
FILL = 0xC3  # the image's fill, another byte than the buffers' sentinel
MPJX_ERR_ARG = -1
BASIC = [MPI.BYTE, MPI.CHAR, MPI.SHORT, MPI.BOOLEAN, MPI.INT, MPI.LONG, MPI.FLOAT, MPI.DOUBLE]
PAIRS = [MPI.SHORT2, MPI.INT2, MPI.LONG2, MPI.FLOAT2, MPI.DOUBLE2]
for _dt in (MPI.SHORT, MPI.FLOAT2):  # the shared case tables name their base types; these two are new to them
    SC.BASES.setdefault(_dt.name, _dt)
PLAIN = IC.PLAIN


@pytest.fixture(scope="module")
def one():
    comms = mpi.smp_world(1, [0])
    yield comms[0]
    comms[0].Free()


def uint(bsz):
    return {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[bsz]


def section(dt, elems):
    """The bytes of one section holding `elems` (base words in pack order): header by hand, payload big-endian."""
    hdr = bytes([dt.baseType - 1, 0, 0, 0]) + struct.pack(">i", elems.size)
    return np.frombuffer(hdr + elems.astype(f">u{dt.baseSize}").tobytes(), dtype=np.uint8)


def source(nelem, bsz, seed):
    raw = np.random.default_rng(seed).integers(0, 256, nelem * bsz, dtype=np.uint8)
    return raw.view(uint(bsz))


def c_pack(one, buf, off, count, dt, image, position, image_bytes=None):
    pos = ctypes.c_int64(position)
    rc = _lib.lib().mpjx_pack(one.handle, buf.data_ptr() + off * dt.baseSize, count, dt.code, image.data_ptr(),
                              image.numel() if image_bytes is None else image_bytes, ctypes.byref(pos), None)
    return rc, pos.value


def c_unpack(one, image, position, buf, off, count, dt, status, image_bytes=None):
    pos = ctypes.c_int64(position)
    rc = _lib.lib().mpjx_unpack(one.handle, image.data_ptr(), image.numel() if image_bytes is None else image_bytes,
                                ctypes.byref(pos), buf.data_ptr() + off * dt.baseSize, count, dt.code,
                                status.data_ptr(), None)
    return rc, pos.value


def sync(one):
    _lib.call("mpjx_comm_synchronize", one.handle)


def round_trip(one, dt, idx, nelem, off, count, position, seed=1, slack=24):
    """Pack `count` items of dt whose packed element indices are idx (from buffer element 0; the call is given
    element `off`) at `position` of a FILL-filled image, unpack into a sentinel buffer; None, or what differs."""
    bsz = dt.baseSize
    src = source(nelem, bsz, seed)
    sec = section(dt, src[idx])
    h = (position + 7) // 8 * 8
    want_img = np.full(h + sec.size + slack, FILL, np.uint8)
    want_img[h:h + sec.size] = sec
    want_out = np.full(nelem * bsz, SENT, np.uint8)
    want_out.view(uint(bsz))[idx] = src[idx]
    dsrc = torch.from_numpy(src.view(np.uint8).copy()).cuda()
    dimg = torch.full((want_img.size,), FILL, dtype=torch.uint8, device="cuda")
    dout = torch.full((nelem * bsz,), SENT, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    what = f"{dt} x{count} @{off} position {position}"
    rc, pos = c_pack(one, dsrc, off, count, dt, dimg, position)
    assert rc == 0, (what, _lib.lib().mpjx_last_error())
    assert pos == h + sec.size, (what, pos, h + sec.size)
    rc, pos = c_unpack(one, dimg, position, dout, off, count, dt, status)
    assert rc == 0, (what, _lib.lib().mpjx_last_error())
    assert pos == h + sec.size, (what, pos)
    sync(one)
    assert int(status.item()) == 0, what
    return (SC.differs(dimg.cpu().numpy(), want_img, what + " (image)")
            or SC.differs(dout.cpu().numpy(), want_out, what + " (unpacked)")
            or SC.differs(dsrc.cpu().numpy(), src.view(np.uint8), what + " (source)"))


@pytest.mark.parametrize("dt", BASIC + PAIRS, ids=lambda d: d.name)
def test_basic_and_pair_types_contiguous(one, dt):
    """Counts 0, 1, 3 and 1025 (1025 crosses one cached tile of 1024 granules where the granule is one element) at
    positions 0 (payload only 8-aligned), 8 (16-aligned) and 5 (header moved to 8). At position 5 the buffer
    starts one element in, which brings the granule down to the element where the element is below 16 B."""
    for count in (0, 1, 3, 1025):
        for position in (0, 8, 5):
            off = 1 if position == 5 else 0
            idx = off + np.arange(count * dt.size, dtype=np.int64)
            assert round_trip(one, dt, idx, count * dt.size + 3, off, count, position, seed=count + position) is None


def test_two_sections_in_one_image(one):
    """BYTE x 3 at 0 returns 11; Vector(3, 2, 5, INT) x 2 from 11 puts its header at 16. Both unpack from there."""
    f = SC.Form("INT", ("V", 3, 2, 5))
    v = f.make()
    try:
        by, ints = source(5, 1, 11), source(40, 4, 12)
        idx = f.index(2, 1)
        want = np.full(16 + 8 + 48 + 8, FILL, np.uint8)
        s1, s2 = section(MPI.BYTE, by[1:4]), section(MPI.INT, ints[idx])
        want[0:s1.size] = s1
        want[16:16 + s2.size] = s2
        dby, dints = torch.from_numpy(by.copy()).cuda(), torch.from_numpy(ints.view(np.uint8).copy()).cuda()
        dimg = torch.full((want.size,), FILL, dtype=torch.uint8, device="cuda")
        oby = torch.full((5,), SENT, dtype=torch.uint8, device="cuda")
        oints = torch.full((160,), SENT, dtype=torch.uint8, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert c_pack(one, dby, 1, 3, MPI.BYTE, dimg, 0) == (0, 11)
        assert c_pack(one, dints, 1, 2, v, dimg, 11) == (0, 72)
        assert c_unpack(one, dimg, 0, oby, 1, 3, MPI.BYTE, status) == (0, 11)
        assert c_unpack(one, dimg, 11, oints, 1, 2, v, status) == (0, 72)
        sync(one)
        assert int(status.item()) == 0
        assert SC.differs(dimg.cpu().numpy(), want, "two sections (image)") is None
        eby, eints = np.full(5, SENT, np.uint8), np.full(160, SENT, np.uint8)
        eby[1:4] = by[1:4]
        eints.view(np.uint32)[idx] = ints[idx]
        assert SC.differs(oby.cpu().numpy(), eby, "BYTE section unpacked") is None
        assert SC.differs(oints.cpu().numpy(), eints, "Vector section unpacked") is None
    finally:
        v.Free()


REV600 = ("I", (1,) * 600, tuple(2 * (599 - i) for i in range(600)))  # above the 512-entry LDS form: direct search
REV300 = ("I", (1,) * 300, tuple(2 * (299 - i) for i in range(300)))  # the LDS form
LAYOUTS = {"vector": (("V", 3, 2, 5), 2), "indexed_SI": (IC.SI, 3), "hindexed_RI_lb1": (IC.RI, 3),
           "hvector_of_vector": ("HV", 2), "reversed_600": (REV600, 2), "reversed_300": (REV300, 2)}


@pytest.mark.parametrize("base", ("INT", "SHORT", "DOUBLE", "FLOAT2"))
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_derived_layouts(one, base, name):
    spec, count = LAYOUTS[name]
    if spec == "HV":  # hvec.java's shape: Hvector(3, 1, 9 items, Vector(2, 3, 4, base))
        spec = ("HV", 3, 1, 9 * SC.BASES[base].size, (2, 3, 4))
    f = IC.form(base, spec)
    t = IC.lib_type(f)
    try:
        for off, position in ((0, 0), (1, 8), (2, 5)):
            idx = f.index(count, off)
            assert idx.size == count * f.size
            assert round_trip(one, t, idx, int(idx.max()) + 3, off, count, position, seed=off + 7) is None
    finally:
        t.Free()


@pytest.mark.parametrize("spec", (("V", 3, 1, 3), ("I", (3, 1, 1), (4, 0, 9)), ("V", 5, 3, 7)), ids=str)
def test_short_with_odd_block_lengths(one, spec):
    """Blocks of an odd number of 2-byte elements: the granule is 2 bytes, one element per lane."""
    f = IC.form("SHORT", spec)
    t = IC.lib_type(f)
    try:
        for off, position in ((0, 0), (1, 8), (0, 5)):
            idx = f.index(7, off)
            assert round_trip(one, t, idx, int(idx.max()) + 3, off, 7, position, seed=3) is None
    finally:
        t.Free()


def test_streaming_form(one, monkeypatch):
    """MPJX_STRIDED_NT_MIN_MIB=1 and a Vector of DOUBLE whose payload is 1 MiB + 8 bytes: the 512-lane
    non-temporal form, 257 tiles, the last one a single granule."""
    monkeypatch.setenv("MPJX_STRIDED_NT_MIN_MIB", "1")
    f = SC.Form("DOUBLE", ("V", 3, 1, 2))
    count = ((1 << 20) + 8) // 8 // 3
    assert count * 3 * 8 == (1 << 20) + 8
    t = f.make()
    try:
        idx = f.index(count, 0)
        assert round_trip(one, t, idx, int(idx.max()) + 2, 0, count, 0) is None
    finally:
        t.Free()


def test_pinned_host_image(one):
    """The image in mpjx_host_alloc memory (a NIC's or the Java side's view): packed by the kernel across the host
    link, checked from the host after synchronising, unpacked from there again."""
    L = _lib.lib()
    f = SC.Form("INT", ("V", 4, 3, 5))
    t = f.make()
    idx = f.index(3, 1)
    src = source(int(idx.max()) + 2, 4, 21)
    sec = section(MPI.INT, src[idx])
    n = 8 + sec.size + 16
    p = ctypes.c_void_p()
    _lib.check(L.mpjx_host_alloc(ctypes.byref(p), n), "mpjx_host_alloc")
    try:
        img = np.frombuffer((ctypes.c_uint8 * n).from_address(p.value), dtype=np.uint8)
        img[:] = FILL
        want = np.full(n, FILL, np.uint8)
        want[8:8 + sec.size] = sec
        dsrc = torch.from_numpy(src.view(np.uint8).copy()).cuda()
        dout = torch.full((src.size * 4,), SENT, dtype=torch.uint8, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        pos = ctypes.c_int64(3)
        assert L.mpjx_pack(one.handle, dsrc.data_ptr() + 4, 3, t.code, p, n, ctypes.byref(pos), None) == 0
        assert pos.value == 8 + sec.size
        sync(one)
        assert SC.differs(img, want, "pinned image") is None
        pos = ctypes.c_int64(3)
        assert L.mpjx_unpack(one.handle, p, n, ctypes.byref(pos), dout.data_ptr() + 4, 3, t.code, status.data_ptr(),
                             None) == 0
        sync(one)
        exp = np.full(src.size * 4, SENT, np.uint8)
        exp.view(np.uint32)[idx] = src[idx]
        assert int(status.item()) == 0 and pos.value == 8 + sec.size
        assert SC.differs(dout.cpu().numpy(), exp, "unpacked from the pinned image") is None
    finally:
        sync(one)
        _lib.check(L.mpjx_host_free(p), "mpjx_host_free")
        t.Free()


def test_malformed_input_to_unpack(one):
    """A wrong type code: status 1; a header count off by one: 2; image_bytes cut short of the expected payload:
    MPJX_ERR_ARG from the host; a header count that overruns the image: 3. outbuf keeps its sentinels every time."""
    L = _lib.lib()
    n = 12
    src = source(n, 4, 5)
    good = np.full(8 + 8 + 4 * n + 16, FILL, np.uint8)
    good[8:16 + 4 * n] = section(MPI.INT, src)

    def attempt(img, count, dt, image_bytes=None):
        dimg = torch.from_numpy(img.copy()).cuda()
        dout = torch.full((4 * n + 8,), SENT, dtype=torch.uint8, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        rc, _ = c_unpack(one, dimg, 8, dout, 0, count, dt, status, image_bytes)
        sync(one)
        assert np.all(dout.cpu().numpy() == SENT), "outbuf was written"
        return rc, int(status.item())

    assert attempt(good, n, MPI.FLOAT) == (0, 1)       # the same word size, another type code
    assert attempt(good, 2 * n, MPI.SHORT) == (0, 1)
    assert attempt(good, n - 1, MPI.INT) == (0, 2)     # the header announces one more than expected
    assert attempt(good, n + 1, MPI.INT) == (0, 2)     # ... one fewer (the image has room for both)
    rc, st = attempt(good, n, MPI.INT, image_bytes=16 + 4 * n - 1)
    assert rc == MPJX_ERR_ARG and st == 0 and b"ends past the image" in L.mpjx_last_error()
    over = good.copy()
    over[12:16] = np.frombuffer(struct.pack(">i", n + 5), dtype=np.uint8)  # 4 * (n + 5) bytes pass the 16 spare ones
    assert attempt(over, n, MPI.INT) == (0, 3)
    neg = good.copy()
    neg[12:16] = 0xFF  # count -1
    assert attempt(neg, n, MPI.INT) == (0, 3)
    # an unpack into a type whose own blocks share a byte
    t = Datatype.Indexed([3, 3], [0, 2], MPI.INT)
    try:
        rc, st = attempt(good, 2, t)
        assert rc == MPJX_ERR_ARG and st == 0 and b"share a byte" in L.mpjx_last_error()
    finally:
        t.Free()


def test_malformed_input_control(one):
    """The control of the test above: the same section, arguments and position, untouched, do unpack."""
    assert round_trip(one, MPI.INT, np.arange(12, dtype=np.int64), 14, 0, 12, 8, seed=5, slack=16) is None


def test_producer_meets_consumer(one):
    """A Vector column of DOUBLE packed into an image that mpjx_mpjbuf_combine(SUM, DOUBLE) then folds into acc:
    acc equals the oracle's SUM of the packed column and the old acc to the bit, status 0."""
    rows, cols = 300, 7
    rng = np.random.default_rng(77)
    m = rng.uniform(-1, 1, rows * cols)
    acc = rng.uniform(-1, 1, rows)
    col = Datatype.Vector(rows, 1, cols, MPI.DOUBLE)
    try:
        dm, dacc = torch.from_numpy(m).cuda(), torch.from_numpy(acc.copy()).cuda()
        dimg = torch.full((8 + 8 * rows,), FILL, dtype=torch.uint8, device="cuda")
        status = torch.zeros(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert c_pack(one, dm, 3, 1, col, dimg, 0) == (0, 8 + 8 * rows)
        sync(one)
        _lib.call("mpjx_mpjbuf_combine", MPI.SUM.opCode, MPI.DOUBLE.code, dacc.data_ptr(), dimg.data_ptr(),
                  dimg.numel(), rows, status.data_ptr(), 0, None)
        torch.cuda.synchronize()
        exp = O.apply(O.SUM, O.DOUBLE, acc.copy(), np.ascontiguousarray(m[3::cols][:rows]))
        assert int(status.item()) == 0
        assert np.array_equal(dacc.cpu().numpy().view(np.uint64), exp.view(np.uint64))
    finally:
        col.Free()


def test_python_mirror(one):
    """Intracomm.Pack / Unpack / Pack_size round-trip a Vector and an Hindexed; Unpack of a bad image raises."""
    assert [one.Pack_size(c, t) for c, t in ((1, MPI.BYTE), (3, MPI.BYTE), (1, MPI.SHORT), (1, MPI.INT),
                                             (1, MPI.DOUBLE))] == [10, 14, 12, 16, 16]
    fv, fh = SC.Form("INT", ("V", 3, 2, 5)), IC.form("DOUBLE", IC.RI)
    v, h = fv.make(), fh.make()
    try:
        assert one.Pack_size(2, v) == 56
        ints, dbl = source(40, 4, 31), source(60, 8, 32)
        iv, ih = fv.index(2, 1), fh.index(3, 2)
        s1, s2 = section(MPI.INT, ints[iv]), section(MPI.DOUBLE, dbl[ih])
        want = np.full(8 + s1.size + s2.size + 8, FILL, np.uint8)
        want[8:8 + s1.size] = s1
        want[8 + s1.size:8 + s1.size + s2.size] = s2  # 56 bytes: the next header is aligned as it is
        dints = torch.from_numpy(ints.view(np.int32).copy()).cuda()
        ddbl = torch.from_numpy(dbl.view(np.float64).copy()).cuda()
        img = torch.full((want.size,), FILL, dtype=torch.uint8, device="cuda")
        pos = one.Pack(dints, 1, 2, v, img, 5)
        assert pos == 8 + s1.size
        pos2 = one.Pack(ddbl, 2, 3, h, img, pos)
        assert pos2 == pos + s2.size
        assert SC.differs(img.cpu().numpy(), want, "mirror image") is None
        oints = torch.full((160,), SENT, dtype=torch.uint8, device="cuda").view(torch.int32)
        odbl = torch.full((480,), SENT, dtype=torch.uint8, device="cuda").view(torch.float64)
        assert one.Unpack(img, 5, oints, 1, 2, v) == pos
        assert one.Unpack(img, pos, odbl, 2, 3, h) == pos2
        eints, edbl = np.full(160, SENT, np.uint8), np.full(480, SENT, np.uint8)
        eints.view(np.uint32)[iv] = ints[iv]
        edbl.view(np.uint64)[ih] = dbl[ih]
        assert SC.differs(oints.view(torch.uint8).cpu().numpy(), eints, "mirror Vector") is None
        assert SC.differs(odbl.view(torch.uint8).cpu().numpy(), edbl, "mirror Hindexed") is None
        keep = torch.full((160,), SENT, dtype=torch.uint8, device="cuda").view(torch.int32)
        with pytest.raises(MPIException, match=r"status 1"):
            one.Unpack(img, pos, keep, 0, 9, MPI.INT)  # a DOUBLE section
        with pytest.raises(MPIException, match=r"status 2"):
            one.Unpack(img, 5, keep, 1, 1, v)  # 12 ints are there, 6 expected
        with pytest.raises(MPIException, match=r"ends past the image"):
            one.Unpack(img, pos2, keep, 0, 9, MPI.INT)
        with pytest.raises(MPIException, match="uint8"):
            one.Pack(dints, 1, 2, v, oints, 0)
        assert np.all(keep.view(torch.uint8).cpu().numpy() == SENT)
        # a pinned image through the mirror
        pimg = torch.full((want.size,), FILL, dtype=torch.uint8).pin_memory()
        assert one.Pack(dints, 1, 2, v, pimg, 5) == pos
        assert SC.differs(pimg.numpy()[:pos], want[:pos], "mirror pinned image") is None
    finally:
        v.Free()
        h.Free()
