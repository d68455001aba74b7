"""Layouts, images and expected bytes of the wire-format message tests (tests/test_gpu_wire.py): every (granule, word)
arm of k_wire over a linear, a Vector and an Indexed layout, with the section built by numpy, independent of the
library: the 8 header bytes, then the layout's elements in pack order, each base word big-endian."""
import numpy as np

from mpjexpress_amd.mpi import MPI, Datatype

SENT = 0xA5
GUARD = 32
WORDS = [(MPI.BYTE, np.int8), (MPI.SHORT, np.int16), (MPI.INT, np.int32), (MPI.DOUBLE, np.float64)]  # by log2 of the word
ARMS = [(g, w) for w in range(4) for g in range(w, 5)]  # (glog, wlog): the 14 arms
KINDS = ("linear", "vector", "indexed")
LENGTHS = (1, 1024, 1025)  # granules: one, one tile of 256 x 4, one tile + 1


class Case:
    """`ngran` granules of 2^glog bytes of words of 2^wlog bytes as ONE item of a type of the kind.
    dt: the library type; count: items; idx: base-element indices from the buffer position, in pack order;
    off: base elements from the start of a 16-aligned tensor to the buffer position (it pins a linear layout's
    granule); span: base elements the tensor must hold from there."""

    def __init__(self, kind, glog, wlog, ngran):
        base, self.np_dtype = WORDS[wlog]
        self.base, self.kind, self.glog, self.wlog, self.ngran = base, kind, glog, wlog, ngran
        self.w = 1 << wlog
        b = self.b = 1 << (glog - wlog)  # words per granule
        self.off = 0
        if kind == "linear":
            self.dt, self.count = base, ngran * b
            self.idx = np.arange(ngran * b, dtype=np.int64)
            self.off = b if glog < 4 else 0
        elif kind == "vector":
            self.dt, self.count = Datatype.Vector(ngran, b, 3 * b, base), 1
            self.idx = (np.arange(ngran, dtype=np.int64)[:, None] * 3 * b + np.arange(b)[None, :]).reshape(-1)
        else:
            ds = [b * (3 * i + (i & 1)) for i in range(ngran)]
            self.dt, self.count = Datatype.Hindexed([b] * ngran, ds, base), 1
            self.idx = (np.asarray(ds, np.int64)[:, None] + np.arange(b)[None, :]).reshape(-1)
        self.words = len(self.idx)
        self.span = int(self.idx.max()) + 1
        self.payload = self.words * self.w

    def free(self):
        if self.dt is not self.base:
            self.dt.Free()

    def values(self, seed):
        """A host array of off + span + GUARD base elements with every byte random."""
        rng = np.random.default_rng(seed)
        n = self.off + self.span + GUARD
        return rng.integers(0, 256, n * self.w, dtype=np.uint8).view(self.np_dtype).copy()

    def blank(self):
        n = self.off + self.span + GUARD
        return np.full(n * self.w, SENT, np.uint8).view(self.np_dtype).copy()


def header(base_code, words):
    return np.array([base_code - 1, 0, 0, 0, (words >> 24) & 255, (words >> 16) & 255, (words >> 8) & 255, words & 255],
                    np.uint8)


def section(base_code, elems):
    """The mpjbuf section of the 1-D array elems (little-endian host order): header and big-endian payload."""
    be = np.ascontiguousarray(elems).byteswap().view(np.uint8)  # bytes only: no value is interpreted
    return np.concatenate([header(base_code, len(elems)), be])


def image(total, at, sec):
    """An image tensor's bytes: `total` sentinel bytes with the section at byte `at`."""
    img = np.full(total, SENT, np.uint8)
    img[at:at + len(sec)] = sec
    return img
