"""The cases that pin every cell of the point-to-point move kernels' per-lane code (csrc/mpjx_k_msgs_tile.hpp, run
by k_msgs and k_msgs_pool), shared by tests/test_gpu_msgs_matrix.py (which runs them on the GPU) and
tests/test_msgs_cases.py (which checks them on the CPU against the planner).

A cell is
  bytes     (sh, tile): both layouts contiguous; sh = (src - dst) & 15 selects the arm of shift16 (q = sh >> 2 the
            dword select, b = sh & 3 the byte alignment); 16 x 2 = 32 cells
  granule   (glog, source form, destination form, tile): one lane moves one granule of 1 << glog bytes; a side is
            "reg" (strided_addr; a contiguous side counts where the other is not) or "irr" (an Indexed type whose
            block table is searched on the device); 5 x 2 x 2 x 2 = 40 cells
and the tile is "default" (256 lanes x 4) or "nt" (the streaming form, 512 lanes x 1, which a launch takes when its
batch carries kStridedStreamBytes of payload: the GPU test puts a 64 MiB ballast message beside the cases).

Everything is over MPI.BYTE, so block lengths, displacements and offsets are bytes. A case is a send Side and a
receive Side (an indexed_cases spec, an item count and the byte offset of the buffer position from a 16-byte aligned
tensor) and the cell it claims. The message is the send side's packed bytes; the receive layout may be longer.
Expected bytes come from numpy indexing of the two layouts alone.

The granule of a case is capped by its layouts: with G = 1 << glog a regular side is blocks of b G bytes at a
stride of (b + 1) G (b or b + 1 is odd), an irregular side has a block of exactly G bytes, and every other block
length, displacement and buffer offset is a multiple of G. `pack_cases.granule_log` restates the rule.
"""
import numpy as np

import indexed_cases as IC
import pack_cases as PC

SENT = 0xA5
TILE = {"default": 1024, "nt": 512}  # kStridedTile, kStridedTileNT: vectors (bytes kind) or granules per tile
TILES = ("default", "nt")
FORMS = ("reg", "irr")
MSGS_MAX = 24                        # kMsgsMax: segments per launch table
STREAM_BYTES = 64 << 20              # kStridedStreamBytes
SLACK = 32                           # sentinel bytes after a layout's last byte
SWEEP_BYTES = 4099                   # whole vectors, a head (but at alignment 0) and a tail (but at alignment 13)
RECV_IRR, RECV_REG = 13, 6           # granules per item of the receive layouts


class Side:
    """`items` items of the BYTE layout `spec` whose origin is byte `off` of the buffer."""

    def __init__(self, spec, items, off):
        self.spec, self.items, self.off = spec, items, off
        self.f = IC.form("BYTE", spec)
        assert spec == IC.PLAIN or (spec[0] == "V" and spec[1] >= 2) or (spec[0] == "I" and len(spec[1]) >= 2), spec

    @property
    def form(self):
        return "irr" if self.spec[0] == "I" else "reg"

    @property
    def contiguous(self):
        return self.spec == IC.PLAIN

    def size(self):
        return self.items * self.f.size

    def index(self):
        """Byte indices of the buffer in pack order."""
        return self.f.index(self.items, self.off)

    def alloc(self):
        """Bytes of the buffer: the layout's span from byte 0, SLACK more, rounded up to 16."""
        return -(-(self.f.span(self.items, self.off) + SLACK) // 16) * 16

    def layout_bytes(self):
        """Every value of the layout that enters the granule."""
        f = self.f
        if self.contiguous:
            return [self.items]
        if self.spec[0] == "V":
            return [f.blocklen, f.stride, f.extent]
        return [v for blk in f.blocks for v in blk] + [f.extent]

    def describe(self):
        """The side as tests/cpp/msgs_plan_test.cpp --cases reads it."""
        s = self.spec
        if self.contiguous:
            args = ["C"]
        elif s[0] == "V":
            args = ["V", *s[1:]]
        else:
            args = ["I", len(s[1]), *s[1], *s[2]]
        return " ".join(str(x) for x in [*args, self.items, self.off])


class Case:
    """claim: ("bytes", sh) or ("granule", glog, source form, destination form)"""

    def __init__(self, name, send, recv, claim, tile, short=False):
        self.name, self.send, self.recv, self.claim, self.tile, self.short = name, send, recv, claim, tile, short
        self.nbytes = send.size()
        assert 0 < self.nbytes <= recv.size(), name

    @property
    def kind(self):
        return self.claim[0]

    @property
    def cell(self):
        return (*self.claim, self.tile)

    @property
    def id(self):
        return f"{self.name}-{self.tile}"

    def describe(self):
        return self.send.describe() + " " + self.recv.describe()

    def source(self, seed):
        return np.random.default_rng(seed).integers(0, 256, self.send.alloc(), dtype=np.uint8)

    def expected(self, src):
        """The whole receive buffer after the message: the sentinel but where the layout puts the packed bytes."""
        exp = np.full(self.recv.alloc(), SENT, np.uint8)
        exp[self.recv.index()[:self.nbytes]] = src[self.send.index()]
        return exp

    def granule(self, sbuf, rbuf):
        """The granule the planner must choose for tensors at sbuf and rbuf, by the restated rule."""
        return PC.granule_log(self.send.layout_bytes() + self.recv.layout_bytes() + [sbuf + self.send.off, rbuf + self.recv.off])

    def shift(self, sbuf, rbuf):
        """(sh, dst & 15) for tensors at sbuf and rbuf."""
        return (sbuf + self.send.off - rbuf - self.recv.off) & 15, (rbuf + self.recv.off) & 15

    def tiles(self, tile=None):
        """Tiles of the segment, from the claim: vectors the destination touches (bytes kind) or granules."""
        t = TILE[tile or self.tile]
        if self.kind == "bytes":
            return -(-((self.recv.off & 15) + self.nbytes + 15 >> 4) // t)
        return -(-(self.nbytes >> self.claim[1]) // t)


# ---- bytes kind ---------------------------------------------------------------------------------------------------

def bytes_case(sh, da, n, tile, what):
    """n bytes to a destination da past a 16-byte line, from a source (da + sh) & 15 past one."""
    return Case(f"sh{sh}-da{da}-{what}", Side(IC.PLAIN, n, 16 + ((da + sh) & 15)), Side(IC.PLAIN, n, 16 + da), ("bytes", sh), tile)


def second_alignment(sh):
    """The non-zero destination alignment of shift sh: every one of 1..15 over the 16 shifts."""
    return 1 + (7 * sh) % 15


def bytes_lengths(tile):
    """what -> bytes, for one destination alignment: one vector, one tile, one tile and a vector, two tiles less
    a byte."""
    t = 16 * TILE[tile]
    return {"vector": 16, "tile": t, "tile+vector": t + 16, "2tiles-1": 2 * t - 1}


def bytes_cases(sh, tile):
    """The nine cases of one bytes cell: 5 B that cross a 16-byte line without a whole vector, and four lengths at
    an aligned destination (no head) and at second_alignment (a head, and a tail but for "2tiles-1" + 1)."""
    out = [bytes_case(sh, 13, 5, tile, "5B")]
    for da in (0, second_alignment(sh)):
        out += [bytes_case(sh, da, n, tile, what) for what, n in bytes_lengths(tile).items()]
    return out


def sweep_cases():
    """All 256 (src & 15, dst & 15) at one length, default tile."""
    return [Case(f"sweep-a{a}-b{b}", Side(IC.PLAIN, SWEEP_BYTES, 16 + a), Side(IC.PLAIN, SWEEP_BYTES, 16 + b),
                 ("bytes", (a - b) & 15), "default") for a in range(16) for b in range(16)]


# ---- granule kind ---------------------------------------------------------------------------------------------------

def granule_counts(tile):
    t = TILE[tile]
    return (1, t - 1, t, t + 1, 2 * t + 1)


def regular_layout(n, G):
    """(spec, items) of exactly n granules: blocks of b >= 2 granules at a stride of b + 1."""
    b = next(x for x in (2, 3, 5, 7) if n % x == 0)
    m = n // b
    c = next((x for x in range(3, m + 1) if m % x == 0), m)
    return ("V", c, b * G, (b + 1) * G), m // c


def shuffled_blocks(p, G, order):
    """An Indexed spec of p granules per item: block lengths 1, 2, 3, 1, 2, 3, ... granules, one granule of gap
    between neighbours in the buffer, packed last block first ("reverse") or odd blocks then even ("riffle"). The
    first block packed is never the buffer's first, so the type stays irregular, and no two abut."""
    lens = []
    while sum(lens) < p:
        lens.append(min((1, 2, 3)[len(lens) % 3], p - sum(lens)))
    offs = [sum(lens[:j]) + j for j in range(len(lens))]
    k = len(lens)
    assert k >= 2
    seq = list(range(k - 1, -1, -1)) if order == "reverse" else list(range(1, k, 2)) + list(range(0, k, 2))
    return ("I", tuple(lens[j] * G for j in seq), tuple(offs[j] * G for j in seq))


def irregular_layout(n, G):
    """(spec, items) of exactly n granules: items of the smallest divisor of n from 8 up."""
    p = next((x for x in range(8, n + 1) if n % x == 0), n)
    return shuffled_blocks(p, G, "reverse"), n // p


def granule_case(glog, sform, dform, n, tile, i, short=False):
    """n granules of 1 << glog bytes from an sform side to a dform side. i varies which regular side is a
    contiguous run and where the buffer positions lie (multiples of the granule, odd ones among them). None where
    no such layout exists: one granule is one block, which is a contiguous run."""
    G = 1 << glog
    if n == 1 and sform == "irr":
        return None
    if sform == "reg" and dform == "reg":
        scon, dcon = (n == 1 or i % 3 == 1), (n > 1 and i % 3 == 2)
    elif sform == "reg":
        scon, dcon = (n == 1 or i % 2 == 1), False
    else:
        scon, dcon = False, (dform == "reg" and i % 2 == 1)
    soff, doff = G * (1, 3, 2, 5, 0)[i % 5], G * (0, 2, 1, 4, 3)[i % 5]
    if scon:
        send = Side(IC.PLAIN, n * G, soff)
    else:
        spec, items = irregular_layout(n, G) if sform == "irr" else regular_layout(n, G)
        send = Side(spec, items, soff)
    if dcon:
        recv = Side(IC.PLAIN, n * G, doff)
    elif dform == "irr":
        recv = Side(shuffled_blocks(RECV_IRR, G, "riffle"), -(-n // RECV_IRR), doff)
    else:
        recv = Side(("V", 3, 2 * G, 3 * G), -(-n // RECV_REG), doff)
    name = f"g{glog}-{sform}-{dform}-n{n}" + ("-short" if short else "")
    return Case(name, send, recv, ("granule", glog, sform, dform), tile, short)


def short_case(glog, tile):
    """One tile exactly, contiguous, into an irregular layout of 13-granule items: the message ends inside the last
    receive item, on the tile's edge."""
    c = granule_case(glog, "reg", "irr", TILE[tile], tile, 1, short=True)
    assert c.send.contiguous and c.nbytes < c.recv.size()
    return c


def granule_cases(glog, tile):
    """Every case of one granule at one tile: its four form pairs at the five counts, and the short case."""
    out = [granule_case(glog, s, d, n, tile, i) for s in FORMS for d in FORMS for i, n in enumerate(granule_counts(tile))]
    return [c for c in out if c] + [short_case(glog, tile)]


# ---- batches ----------------------------------------------------------------------------------------------------------

FULL_TABLE = MSGS_MAX + 1


def full_table():
    """25 segments, bytes and granule kinds in turn, of one tile (1) and of three (S) in the order 1 S S 1 1 S S 1
    ..., so that the prefix search meets every pair of neighbours. Default tile; two launch tables."""
    out = []
    for k in range(FULL_TABLE):
        several = k % 4 in (1, 2)
        if k % 2 == 0:
            sh, da = (5 * k + 1) % 16, (3 * k) % 16
            out.append(bytes_case(sh, da, 40000 if several else 1000 + k, "default", f"full{k}"))
        else:
            glog, (s, d) = (k // 2) % 5, (("reg", "irr"), ("irr", "reg"), ("irr", "irr"), ("reg", "reg"))[(k // 2) % 4]
            c = granule_case(glog, s, d, 2500 if several else 300, "default", k)
            c.name = f"full{k}-" + c.name
            out.append(c)
    return out


def pool_cases(tile):
    """What the persistent requests repeat: every shift (a tile and a vector, with a head and a tail) and the
    irregular-to-irregular row of every granule (one granule past a tile)."""
    t = TILE[tile]
    rows = [granule_case(glog, "irr", "irr", t + 1, tile, glog) for glog in range(5)]
    for c in rows:
        c.name = "pool-" + c.name
    return [bytes_case(sh, second_alignment(sh), 16 * t + 16, tile, "pool") for sh in range(16)] + rows


def all_cases():
    out = []
    for tile in TILES:
        for sh in range(16):
            out += bytes_cases(sh, tile)
        for glog in range(5):
            out += granule_cases(glog, tile)
        out += pool_cases(tile)
    return out + sweep_cases() + full_table()
