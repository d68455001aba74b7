"""GPU: every cell of k_pack (csrc/mpjx_k_pack.hip) through mpjx_pack / mpjx_unpack on device 0.

tests/pack_cases.py holds the cases: for each of the 14 arms (granule, base word) of the kernel's switch one
layout per address form (linear, regular strided, irregular searched in LDS, irregular searched in the device
table), at the default tile and at the streaming tile, by two independent routes to the arm where the granule is
below 16 bytes. tests/test_pack_cases.py proves on the CPU, against the planner, that the cases cover all 224
cells; here each one runs through test_gpu_pack.round_trip: the expected image is built with numpy from the case's
own element index (header by hand, `.astype('>u…')` payload, seeded random bytes) and three whole buffers are
compared byte for byte — the image with its FILL surround, the unpack target with its sentinel gaps, the source.

A case cannot quietly run another arm: round_trip's two library calls are wrapped so that, with the REAL device
pointers in hand, the granule is recomputed by the rule restated in pack_cases.granule_log and must equal the
case's claim, and the torch allocations must be 16-byte aligned as the case table assumes.

No test provokes a fault: every address a case touches lies inside the buffers allocated here (the census checks
the layouts' spans against them), and the malformed images are rejected by the kernel's header check before any
payload load; the host has already checked that the expected payload lies inside the image.
"""
import struct

import numpy as np
import pytest

import indexed_cases as IC
import pack_cases as PC
import test_gpu_pack as TP
from mpjexpress_amd.mpi import MPI
from test_gpu_pack import FILL, SENT, c_unpack, one, round_trip, section, source, sync  # noqa: F401 (one: fixture)

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KNOBS = ("MPJX_STRIDED_NT_MIN_MIB", "MPJX_INDEXED_LDS_MAX_BLOCKS")


def run_case(one, monkeypatch, c, t, seed):
    """round_trip of case c with its knobs set and its claimed granule checked against the real pointers of both
    calls; None, or what differs, named by the cell."""
    calls = []

    def check(buf, image, off, position):
        assert buf.data_ptr() % 16 == 0 and image.data_ptr() % 16 == 0, (c.id, "a torch allocation is not 16-byte aligned")
        assert (off, position) == (c.off, c.position), c.id
        g = c.glog(buf.data_ptr(), image.data_ptr())
        assert g == c.arm[0], (c.id, f"the pointers give granule {1 << g} B, the case claims {1 << c.arm[0]} B")
        calls.append(g)

    real_pack, real_unpack = TP.c_pack, TP.c_unpack

    def pack(one, buf, off, count, dt, image, position, image_bytes=None):
        check(buf, image, off, position)
        return real_pack(one, buf, off, count, dt, image, position, image_bytes)

    def unpack(one, image, position, buf, off, count, dt, status, image_bytes=None):
        check(buf, image, off, position)
        return real_unpack(one, image, position, buf, off, count, dt, status, image_bytes)

    with monkeypatch.context() as m:
        for k in KNOBS:
            m.delenv(k, raising=False)
        for k, v in c.env().items():
            m.setenv(k, v)
        m.setattr(TP, "c_pack", pack)
        m.setattr(TP, "c_unpack", unpack)
        r = round_trip(one, t, c.index(), c.nelem(), c.off, c.count, c.position, seed=seed, slack=PC.IMAGE_SLACK)
    assert len(calls) == 2, c.id
    return r and f"cell g{c.arm[0]}w{c.arm[1]} {c.form} {c.tile} ({c.id}): {r}"


def run_cases(one, monkeypatch, cases):
    types, bad = {}, []
    try:
        for seed, c in enumerate(cases, 1):
            key = (c.base, c.spec)
            if key not in types:
                types[key] = IC.lib_type(c.f)
            bad.append(run_case(one, monkeypatch, c, types[key], seed))
    finally:
        for (_, spec), t in types.items():
            if spec != IC.PLAIN:
                t.Free()
    return [b for b in bad if b]


@pytest.mark.parametrize("arm", PC.ARMS, ids=lambda a: f"g{a[0]}w{a[1]}")
def test_arm(one, monkeypatch, arm):
    """One arm of the switch in its four address forms, packed and unpacked, at the default tile (granule counts
    around 256, 1024 and 2048) and at the streaming tile (1 MiB and a last tile of 1 to 3 granules)."""
    bad = run_cases(one, monkeypatch, PC.arm_cases(arm))
    assert not bad, "\n".join(bad)


def test_lds_capacity_edge(one, monkeypatch):
    """Reversed one-element blocks of INT: 512 of them are searched in LDS (every lane of the 512-lane kernel
    fills one entry, every lane of the 256-lane kernel two), 513 in the device table; both tiles."""
    bad = run_cases(one, monkeypatch, PC.edge_cases())
    assert not bad, "\n".join(bad)


def unpack_attempt(one, img, n, dt):
    """Unpack n elements of basic type dt from position 8 of img into a sentinel buffer: (rc, status, outbuf)."""
    dimg = torch.from_numpy(img.copy()).cuda()
    dout = torch.full((n * dt.baseSize + 16,), SENT, dtype=torch.uint8, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc, _ = c_unpack(one, dimg, 8, dout, 0, n, dt, status)
    sync(one)
    return rc, int(status.item()), dout.cpu().numpy()


def with_count(img, n):
    out = img.copy()
    out[12:16] = np.frombuffer(struct.pack(">i", n), dtype=np.uint8)
    return out


def good_image(dt, n, spare, seed):
    """A section of n elements of dt at position 8 (header at 8, payload at 16) and `spare` FILL bytes after it."""
    src = source(n, dt.baseSize, seed)
    img = np.full(16 + n * dt.baseSize + spare, FILL, np.uint8)
    img[8:16 + n * dt.baseSize] = section(dt, src)
    return src, img


@pytest.mark.parametrize("tile, n", (("default", 3073), ("nt", (1 << 20) // 4 + 3)), ids=("default", "nt"))
def test_bad_header_ends_every_block(one, monkeypatch, tile, n):
    """An INT section of more than three tiles (3073 granules of 4 B at 1024 a tile; 1 MiB + 12 B at 512 a tile)
    whose header is wrong: status 1, 2 or 3, and NO block of the grid stores a byte. The unmodified image
    unpacks."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    if tile == "nt":
        monkeypatch.setenv("MPJX_STRIDED_NT_MIN_MIB", "1")
    spare = 16
    src, good = good_image(MPI.INT, n, spare, 9)
    assert PC.granule_log([4 * n]) == 2 and n > 3 * (512 if tile == "nt" else 1024)
    wrong_type = good.copy()
    wrong_type[8] = MPI.FLOAT.baseType - 1
    for img, want in ((wrong_type, 1), (with_count(good, n + 1), 2), (with_count(good, n - 1), 2),
                      (with_count(good, n + spare // 4 + 1), 3), (with_count(good, -1), 3)):
        rc, st, out = unpack_attempt(one, img, n, MPI.INT)
        assert (rc, st) == (0, want), (tile, want)
        assert np.all(out == SENT), (tile, want, f"{np.count_nonzero(out != SENT)} bytes of outbuf were written, the "
                                     f"first at byte {np.flatnonzero(out != SENT)[0]}")
    rc, st, out = unpack_attempt(one, good, n, MPI.INT)
    exp = np.full(out.size, SENT, np.uint8)
    exp[:4 * n] = src.view(np.uint8)
    assert (rc, st) == (0, 0) and np.array_equal(out, exp)


@pytest.mark.parametrize("dt", (MPI.BYTE, MPI.SHORT, MPI.INT, MPI.DOUBLE), ids=lambda d: d.name)
def test_overrun_boundary_per_word_size(one, monkeypatch, dt):
    """16 spare bytes of image after the payload: a header count whose payload ends exactly at the image's end is
    only the wrong count (status 2), one base word more passes the end (status 3). Pins n << wlog per wlog."""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    n, spare, w = 7, 16, dt.baseSize
    src, good = good_image(dt, n, spare, 13)
    for count, want in ((n + spare // w, 2), (n + spare // w + 1, 3), (n + spare // w - 1, 2)):
        rc, st, out = unpack_attempt(one, with_count(good, count), n, dt)
        assert (rc, st) == (0, want), (dt.name, count, st, want)
        assert np.all(out == SENT), (dt.name, count)
    rc, st, out = unpack_attempt(one, good, n, dt)
    exp = np.full(out.size, SENT, np.uint8)
    exp[:w * n] = src.view(np.uint8)
    assert (rc, st) == (0, 0) and np.array_equal(out, exp), dt.name
