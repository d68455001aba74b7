"""The cases that pin every cell of k_pack (csrc/mpjx_k_pack.hip), shared by tests/test_gpu_pack_matrix.py (which
runs them on the GPU) and tests/test_pack_cases.py (which checks them on the CPU against the planner).

A cell is (glog, wlog, form): the arm of the kernel's switch (granule G = 1 << glog bytes of words of
W = 1 << wlog bytes, 14 arms) and where the buffer-side address comes from:
  lin     the layout is one contiguous run            reg     strided_addr
  lds     the block table copied to LDS               direct  the device table searched where it lies
Each cell exists in four kernels (pack or unpack, the 256 x 4 default tile or the 512 x 1 non-temporal tile):
every case is packed AND unpacked, and carries the tile it claims.

With e = G / W elements per granule a case is built so that the lowest set bit of the OR of every block length,
block offset, stride, extent (all in bytes), the buffer address and the payload address is exactly G, by one
of three ROUTES:
  lengths  every block is e elements long (a contiguous run: an odd number of granules); the buffer and the
           payload are 16-byte aligned
  offset   every block and offset is a multiple of 2e elements (a contiguous run: an even number of granules);
           the call is given buffer element e
  payload  (G = 8 only) everything is 16-byte aligned but the payload, which at position 0 starts at image + 8
The layouts are the basic type, Vector(c, u, 3u) and Indexed over the patterns of IRR scaled by u (u: the
items that make one block); c and the pattern are chosen to divide the case's granule count.

`granule_log` is the rule the kernel's planner must follow, restated here from the format's definition and
independent of the library; the GPU test applies it to the real device pointers.
"""
import indexed_cases as IC
import strided_cases as SC
from mpjexpress_amd.mpi import MPI

for _dt in (MPI.SHORT, MPI.FLOAT2):  # the shared case tables name their base types; these two are new to them
    SC.BASES.setdefault(_dt.name, _dt)

ARMS = [(g, w) for w in range(4) for g in range(w, 5)]  # (glog, wlog): the 14 arms of k_pack's switch
WORD_BASE = ("BYTE", "SHORT", "INT", "DOUBLE")          # the base type of word 1 << wlog
FORMS = ("lin", "reg", "lds", "direct")
TILES = ("default", "nt")
TILE_COUNTS = (255, 256, 257, 1023, 1024, 1025, 2049)   # around one, two and four default tiles of 1024, and of 256 lanes
NT_BYTES = 1 << 20       # MPJX_STRIDED_NT_MIN_MIB=1, the smallest the knob allows
NT_TILE = 512
LDS_BLOCKS = 512         # the largest table the LDS form holds
IMAGE_SLACK = 24         # FILL bytes after a section in the image (round_trip's default)

# granules per item -> (block lengths, displacements) in blocks' units: offsets go back and forth, the first is
# not 0 (so none normalises to a Vector), no two blocks abut
IRR = {2: ((1, 1), (3, 0)), 3: ((2, 1), (4, 0)), 5: ((3, 2), (4, 0)), 6: IC.SI[1:],
       257: ((1,) * 257, tuple(2 * (256 - i) for i in range(257)))}


def granule_log(values):
    """log2 of the largest power of two <= 16 that divides every value: the lowest set bit of their OR."""
    m = 16
    for v in values:
        m |= v
    return (m & -m).bit_length() - 1


def reversed_blocks(n):
    """n one-element blocks two elements apart, the last of the buffer first: a wrong search shows."""
    return ("I", (1,) * n, tuple(2 * (n - 1 - i) for i in range(n)))


class Case:
    def __init__(self, arm, form, base, spec, count, off, position, ngran, tile, route):
        self.arm, self.form, self.base, self.spec = arm, form, base, spec
        self.count, self.off, self.position, self.ngran, self.tile, self.route = count, off, position, ngran, tile, route
        self.f = IC.form(base, spec)
        self.bsz = self.f.bsz

    @property
    def cell(self):
        return (self.arm[0], self.arm[1], self.form)

    @property
    def id(self):
        return (f"g{self.arm[0]}w{self.arm[1]}-{self.form}-{self.tile}-{self.route}-{self.base}"
                f"-n{self.ngran}")

    def env(self):
        """The knobs the case runs under (both are read per call)."""
        e = {}
        if self.tile == "nt":
            e["MPJX_STRIDED_NT_MIN_MIB"] = "1"
        if self.form == "direct" and self.nblocks() <= LDS_BLOCKS:
            e["MPJX_INDEXED_LDS_MAX_BLOCKS"] = "0"
        return e

    def nblocks(self):
        return len(self.f.blocks) if self.spec[0] == "I" else self.f.nblocks

    def index(self):
        return self.f.index(self.count, self.off)

    def nelem(self):
        """Base elements of the buffers: the layout's span from element 0 and two spare elements."""
        return self.f.span(self.count, self.off) + 2

    def layout_bytes(self):
        """Every value of the layout that enters the granule, in bytes."""
        f, b = self.f, self.bsz
        if self.spec == IC.PLAIN:
            return [self.count * f.size * b]
        if self.spec[0] == "V":
            return [f.blocklen * b, f.stride * b, f.extent * b]
        return [v * b for blk in f.blocks for v in blk] + [f.extent * b]

    def addresses(self, buf, image):
        """(buffer address the call is given, payload address) for allocations at `buf` and `image`."""
        return buf + self.off * self.bsz, image + (self.position + 7) // 8 * 8 + 8

    def glog(self, buf, image):
        return granule_log(self.layout_bytes() + list(self.addresses(buf, image)))

    def describe(self):
        """The case as tests/cpp/pack_plan_test.cpp --cases reads it: base code, constructor, its arguments,
        count, buffer offset (base elements), position."""
        s = self.spec
        if s == IC.PLAIN:
            args = ["B", 0]
        elif s[0] == "V":
            args = ["V", 3, *s[1:]]
        else:
            args = ["I", 2 * len(s[1]), *s[1], *s[2]]
        return " ".join(str(x) for x in [self.f.base.code, *args, self.count, self.off, self.position])


def make(arm, form, base, ngran, tile, route, p=None):
    """The case of `ngran` granules on `arm` in `form`, or None where the route's layout does not admit ngran."""
    glog, wlog = arm
    G = 1 << glog
    e = G >> wlog                       # base elements per granule
    per = SC.BASES[base].size           # 2 for a pair type
    m = 1 if route == "lengths" else 2  # granules per block unit
    off = e if route == "offset" else 0
    position = 0 if route == "payload" else 8
    assert G < 16 or route == "lengths"
    assert route != "payload" or G == 8
    assert (m * e) % per == 0
    if form == "lin":
        if m == 1 and G < 16 and ngran % 2 == 0:
            return None  # an even count of granules makes the length a multiple of 2G
        if m == 2 and ngran % 2:
            return None  # the other routes need a length of a multiple of 2G
        return Case(arm, form, base, IC.PLAIN, ngran * e // per, off, position, ngran, tile, route)
    if ngran % m:
        return None
    want = (p,) if p else ((3, 2, 5, 257) if form == "reg" else (6, 3, 2, 5, 257))
    p = next((x for x in want if (ngran // m) % x == 0), None)
    if p is None:
        return None
    u = m * e // per  # items per block unit
    if form == "reg":
        spec = ("V", p, u, 3 * u)
    else:
        spec = ("I", tuple(x * u for x in IRR[p][0]), tuple(x * u for x in IRR[p][1]))
    return Case(arm, form, base, spec, ngran // (m * p), off, position, ngran, tile, route)


def nt_case(arm, form, base):
    """The smallest payload of at least 1 MiB whose last 512-lane tile holds the 1, 2 or 3 granules the arm's turn
    gives it (a contiguous run below 16 B needs an odd count, the six-granule Indexed item an even one)."""
    i = ARMS.index(arm)
    tail = (1, 3)[i % 2] if form == "lin" else 1 + i % 3 if form == "reg" else 2
    n = NT_BYTES >> arm[0]
    while True:
        if n % NT_TILE == tail:
            c = make(arm, form, base, n, "nt", "lengths", p=None if form == "lin" else (3 if form == "reg" else 6))
            if c:
                return c
        n += 1


def arm_cases(arm):
    """Every case of one arm: its four forms at both tiles, by both routes where G < 16."""
    i = ARMS.index(arm)
    G = 1 << arm[0]
    out = []
    for base in [WORD_BASE[arm[1]]] + (["FLOAT2"] if arm in ((3, 2), (4, 2)) else []):
        for k, form in enumerate(FORMS):
            if base == "FLOAT2" and form == "lin":
                continue  # a pair swaps its base word: the derived forms show it
            n = TILE_COUNTS[(i + 2 * k + (3 if base == "FLOAT2" else 0)) % 7]
            c = make(arm, form, base, n, "default", "lengths") or make(arm, form, base, n, "default", "offset")
            assert c, (arm, form, n)
            out.append(c)
            if G < 16 and base != "FLOAT2":  # the second route to the same arm
                if c.route == "offset":  # a contiguous run of an even count: the lengths cap an odd one
                    c2 = make(arm, form, base, (255, 257, 1023, 1025, 2049)[i % 5], "default", "lengths")
                else:
                    c2 = make(arm, form, base, (256, 1024)[(i + k) % 2], "default", "offset")
                assert c2, (arm, form)
                out.append(c2)
            out.append(nt_case(arm, form, base))
        if G == 8 and base != "FLOAT2":
            out.append(make(arm, "lin", base, (256, 1024)[i % 2], "default", "payload"))
    return out


def all_cases():
    return [c for arm in ARMS for c in arm_cases(arm)]


def edge_cases():
    """The LDS capacity edge: exactly 512 reversed one-element blocks (the LDS form) and 513 (the direct search),
    over INT, at three default tiles and at 1 MiB and above in the streaming form."""
    out = []
    for nb, form in ((LDS_BLOCKS, "lds"), (LDS_BLOCKS + 1, "direct")):
        for tile, count in (("default", 5), ("nt", (NT_BYTES // 4 + nb - 1) // nb + 1)):
            out.append(Case((2, 2), form, "INT", reversed_blocks(nb), count, 0, 8, count * nb, tile, "lengths"))
    return out
