"""CPU: Datatype.Struct, the LB / UB markers and explicit bounds on every constructor (no GPU).

  - tests/golden/lbub_kat.json: the ten Struct types of the reference's test/mpi/dtyp/lbub.java and lbub2.java
    through mpjx_type_struct, mpjx_type_info and mpjx_type_layout.
  - an independent restatement, in Python, of Struct.computeBounds (src/mpi/Struct.java:149-386, as written) and of
    the older constructors' bounds over an oldtype with explicit bounds, compared with the library on a few
    hundred random small types with fixed seeds; permutations of one Struct's components show that the bounds
    depend on their order.
  - errors, normalisation, the Python mirror, include/mpjx.hpp, and that none of it needs a device.
"""
import ctypes
import itertools
import json
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "mpjx.h")
KAT = os.path.join(ROOT, "tests", "golden", "lbub_kat.json")
ERR_ARG, ERR_UNSUPPORTED = -1, -6
BYTE, INT, DOUBLE, DOUBLE2, LB, UB = 1, 5, 8, 0x108, 10, 11


@pytest.fixture(scope="module")
def L():
    from mpjexpress_amd import _lib

    return _lib.lib()


def arr(v):
    return (ctypes.c_int64 * max(len(v), 1))(*v)


def struct(L, bl, disp, types):
    code = ctypes.c_int(-1)
    rc = L.mpjx_type_struct(len(bl), arr(bl), arr(disp), (ctypes.c_int * max(len(types), 1))(*types), ctypes.byref(code))
    return rc, code.value


def made(r):
    assert r[0] == 0 and r[1] >= 0x10000, r
    return r[1]


def layout(L, code):
    """(base, size, extent, lb, ub, merged blocks, regular) of a live code."""
    base, size, extent = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64()
    lb, ub, nb, reg = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int(-1)
    assert L.mpjx_type_info(code, ctypes.byref(base), ctypes.byref(size), ctypes.byref(extent)) == 0
    assert L.mpjx_type_layout(code, ctypes.byref(lb), ctypes.byref(ub), ctypes.byref(nb), ctypes.byref(reg)) == 0
    return base.value, size.value, extent.value, lb.value, ub.value, nb.value, reg.value


def bounds(L, code):
    return layout(L, code)[2:5]


def one(L, fn, *args):
    code = ctypes.c_int(-1)
    assert getattr(L, fn)(*args, ctypes.byref(code)) == 0, L.mpjx_last_error()
    return code.value


# ---- the known answers ---------------------------------------------------------------------------------------

def test_lbub_known_answers(L):
    kat = json.load(open(KAT))
    assert len(kat["cases"]) == 10
    names = {"INT": INT, "LB": LB, "UB": UB}
    for n, t in kat["types"].items():
        assert t["constructor"] == "Contiguous"
        names[n] = one(L, "mpjx_type_contiguous", t["count"], names[t["oldtype"]])
    for c in kat["cases"]:
        code = made(struct(L, c["blocklengths"], c["displacements"], [names[t] for t in c["types"]]))
        assert bounds(L, code) == (c["extent"], c["lb"], c["ub"]), (c["source"], c["name"])
        assert layout(L, code)[0] == INT
        assert L.mpjx_type_free(code) == 0
    seen = {(c["extent"], c["lb"], c["ub"]) for c in kat["cases"]}
    assert {(97, 0, 97), (98, 0, 98), (91, 3, 94), (99, -3, 96), (89, -3, 86), (100, 0, 100), (33, 65, 98)} == seen


# ---- the restatement -------------------------------------------------------------------------------------------

class Ref:
    """A type as the reference keeps it: size, lb, ub, the two flags (extent = ub - lb), and its code here."""

    def __init__(self, size, lb, ub, lbs, ubs, code):
        self.size, self.lb, self.ub, self.lbs, self.ubs, self.code = size, lb, ub, lbs, ubs, code

    @property
    def extent(self):
        return self.ub - self.lb


def ref_basic(code):
    if code == LB:
        return Ref(0, 0, 0, True, False, code)
    if code == UB:
        return Ref(0, 0, 0, False, True, code)
    return Ref(2 if code == DOUBLE2 else 1, 0, 2 if code == DOUBLE2 else 1, False, False, code)


def ref_struct(bl, disp, types):
    """Struct.computeBounds, statement by statement (Struct.java:155-385)."""
    INF = float("inf")
    lbs = ubs = False
    lb, ub, true_lb, true_ub = INF, -INF, INF, -INF
    for n, d, t in zip(bl, disp, types):
        if n <= 0 or not (t.size != 0 or t.lbs or t.ubs):
            continue
        max_ub = d + (n - 1) * t.extent + t.ub
        if t.ubs:
            ubs = True
            ub = max_ub
        elif max_ub > true_ub:
            true_ub = max_ub
            ub = max_ub if max_ub > d else d
        min_lb = d + t.lb
        if t.lbs:
            lbs = True
            lb = min_lb
        elif min_lb < true_lb:
            true_lb = min_lb
            lb = min_lb if min_lb < d else d
    if lb == INF and ub == -INF:
        lb = ub = 0
    return sum(n * t.size for n, t in zip(bl, types)), lb, ub, lbs, ubs


def ref_minmax(blocks, old):
    """Indexed.computeBounds over (length, start) blocks; Vector's and Contiguous' closed forms are this for the
    positive strides the library builds (Vector.java:124-128, Contiguous.java:94-97)."""
    live = [(n, s) for n, s in blocks if n > 0]
    reps = sum(n for n, _ in live)
    if not live or not (old.size != 0 or old.lbs or old.ubs):
        return reps * old.size, 0, 0, False, False
    lb = min(s + old.lb for _, s in live)
    ub = max(s + (n - 1) * old.extent + old.ub for n, s in live)
    return reps * old.size, lb, ub, old.lbs, old.ubs


def check(L, code, want, what):
    size, lb, ub = want[0], want[1], want[2]
    got = layout(L, code)
    assert (got[1], got[2], got[3], got[4]) == (size, ub - lb, lb, ub), (what, got, want)


def random_struct(rng, L, pool):
    n = rng.randint(1, 5)
    types = [rng.choice(pool) for _ in range(n)]
    bl = [rng.randint(0, 3) for _ in range(n)]
    disp = [rng.randint(-6, 30) if t.size == 0 else rng.randint(0, 30) for t in types]
    return bl, disp, types


def test_struct_bounds_match_the_restatement_on_random_types(L):
    rng = random.Random(0x5757)
    made_codes, checked, unsupported = [], 0, 0
    c4 = Ref(4, 0, 4, False, False, one(L, "mpjx_type_contiguous", 4, INT))
    v = Ref(6, 0, 8, False, False, one(L, "mpjx_type_vector", 3, 2, 3, INT))
    pool = [ref_basic(INT), ref_basic(LB), ref_basic(UB), c4, v]
    for _ in range(400):
        bl, disp, types = random_struct(rng, L, pool)
        want = ref_struct(bl, disp, types)
        rc, code = struct(L, bl, disp, [t.code for t in types])
        if want[2] < want[1]:  # an explicit extent below 0: refused, and the message names it
            assert rc == ERR_UNSUPPORTED and b"extent" in L.mpjx_last_error(), (bl, disp, want)
            assert str(want[2] - want[1]).encode() in L.mpjx_last_error()
            unsupported += 1
            continue
        assert rc == 0, (bl, disp, L.mpjx_last_error())
        check(L, code, want, (bl, disp, [t.code for t in types]))
        checked += 1
        made_codes.append(code)
        if len(pool) < 12 and want[0] > 0 and (want[3] or want[4]):  # feed types with sticky bounds back in
            pool.append(Ref(*want, code))
    assert checked > 250 and unsupported > 5
    assert sum(1 for t in pool if t.lbs or t.ubs) > 3


def test_older_constructors_over_a_resized_oldtype(L):
    rng = random.Random(0x1B0B)
    olds = []
    for bl, disp, types in (([1, 1], [0, 1], [INT, UB]),            # an INT resized to... its own extent
                            ([1, 1], [0, 3], [INT, UB]),            # padded to 3
                            ([2, 1, 1], [1, -2, 7], [INT, LB, UB]),  # lb -2, ub 7
                            ([3, 1], [0, 1], [INT, UB]),            # items interleave: extent 1, data 3
                            ([1, 1], [2, 2], [INT, UB]),            # extent 0... lb 2 = ub 2
                            ([1, 1], [4, 0], [DOUBLE2, LB])):
        refs = [ref_basic(t) for t in types]
        want = ref_struct(bl, disp, refs)
        code = made(struct(L, bl, disp, types))
        check(L, code, want, ("Struct", bl, disp, types))
        olds.append(Ref(*want, code))
    n = 0
    for old in olds:
        for _ in range(12):
            count, blen, stride = rng.randint(0, 4), rng.randint(0, 3), rng.randint(1, 6)
            code = ctypes.c_int(-1)
            # Contiguous
            assert L.mpjx_type_contiguous(count, old.code, ctypes.byref(code)) == 0, L.mpjx_last_error()
            check(L, code.value, ref_minmax([(count, 0)], old), ("Contiguous", count, old.code))
            # Vector: stride in extents of old; Hvector: in base elements
            rs = stride * old.extent
            for fn, real in (("mpjx_type_vector", rs), ("mpjx_type_hvector", stride)):
                rc = getattr(L, fn)(count, blen, stride, old.code, ctypes.byref(code))
                if count > 1 and real < 1 and blen > 0:
                    assert rc == ERR_UNSUPPORTED, (fn, count, blen, stride)
                    continue
                assert rc == 0, (fn, L.mpjx_last_error())
                blocks = [(blen, j * real) for j in range(count)]
                check(L, code.value, ref_minmax(blocks, old), (fn, count, blen, stride, old.code))
            # Indexed (extents of old) and Hindexed (base elements)
            k = rng.randint(1, 4)
            bls, ds = [rng.randint(0, 3) for _ in range(k)], [rng.randint(0, 9) for _ in range(k)]
            for fn, unit in (("mpjx_type_indexed", old.extent), ("mpjx_type_hindexed", 1)):
                assert getattr(L, fn)(k, arr(bls), arr(ds), old.code, ctypes.byref(code)) == 0, L.mpjx_last_error()
                check(L, code.value, ref_minmax([(b, d * unit) for b, d in zip(bls, ds)], old), (fn, bls, ds, old.code))
            n += 1
    assert n == 72


def test_marker_order_changes_the_bounds(L):
    """One set of components, every order: MPI's sticky minimum / maximum would give one answer; the reference gives
    several, and the library gives the reference's for each."""
    comps = [(1, 0, INT), (1, 20, UB), (1, 12, UB), (1, 30, INT), (1, 5, LB)]
    answers = set()
    for perm in itertools.permutations(comps):
        bl, disp, types = [c[0] for c in perm], [c[1] for c in perm], [c[2] for c in perm]
        want = ref_struct(bl, disp, [ref_basic(t) for t in types])
        code = made(struct(L, bl, disp, types))
        check(L, code, want, perm)
        answers.add(bounds(L, code))
        assert L.mpjx_type_free(code) == 0
    assert len(answers) >= 3, answers
    # the later marker wins (Struct.java:242-244), and a data block after it moves ub again (:251-258)
    assert bounds(L, made(struct(L, [1, 1, 1], [0, 20, 12], [INT, UB, UB]))) == (12, 0, 12)
    assert bounds(L, made(struct(L, [1, 1, 1], [0, 12, 20], [INT, UB, UB]))) == (20, 0, 20)
    assert bounds(L, made(struct(L, [1, 1, 1], [0, 12, 30], [INT, UB, INT]))) == (31, 0, 31)
    assert bounds(L, made(struct(L, [1, 1, 1], [0, 30, 12], [INT, INT, UB]))) == (12, 0, 12)
    # a marker is an unmarked component for the other bound: an LB before any data sets ub too
    assert bounds(L, made(struct(L, [1, 1], [10, 0], [LB, INT]))) == (10, 0, 10)


# ---- normalisation, layout ------------------------------------------------------------------------------------

def test_a_regular_struct_is_the_vector(L):
    v = one(L, "mpjx_type_vector", 6, 2, 5, INT)
    s = made(struct(L, [2] * 6, [5 * i for i in range(6)], [INT] * 6))
    assert layout(L, s) == layout(L, v) == (INT, 12, 27, 0, 27, 6, 1)
    # a resized column: the Vector's blocks, extent 1, still regular
    col = made(struct(L, [1, 1], [0, 1], [one(L, "mpjx_type_vector", 7, 1, 9, DOUBLE), UB]))
    assert layout(L, col) == (DOUBLE, 7, 1, 0, 1, 7, 1)
    tlb, tub = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert L.mpjx_type_true_bounds(col, ctypes.byref(tlb), ctypes.byref(tub)) == 0
    assert (tlb.value, tub.value) == (0, 55)
    # abutting components merge; empty ones are dropped; pack order is the arrays' order
    m = made(struct(L, [2, 0, 3, 1], [0, 50, 2, 9], [INT, INT, INT, INT]))
    assert layout(L, m) == (INT, 6, 10, 0, 10, 2, 0)
    back = made(struct(L, [2, 2], [2, 0], [INT, INT]))
    assert layout(L, back) == (INT, 4, 4, 0, 4, 2, 0)
    gap = made(struct(L, [1, 2], [0, 3], [INT, INT]))
    assert layout(L, gap) == (INT, 3, 5, 0, 5, 2, 0)
    empty = made(struct(L, [], [], []))
    assert layout(L, empty)[1:5] == (0, 0, 0, 0)
    only = made(struct(L, [1, 1], [-4, 9], [LB, UB]))
    # markers only: the UB, an unmarked component for lb and the first of those, moves lb to itself (Struct.java:291-298)
    assert layout(L, only)[1:5] == (0, 0, 9, 9)
    assert layout(L, made(struct(L, [1, 1, 1], [0, -4, 9], [INT, LB, UB])))[1:5] == (1, 13, -4, 9)
    pair = made(struct(L, [2, 1], [0, 6], [DOUBLE2, DOUBLE2]))
    assert layout(L, pair) == (DOUBLE, 6, 8, 0, 8, 2, 0)
    mixed = made(struct(L, [1, 1], [0, 2], [DOUBLE2, DOUBLE]))  # one base type: DOUBLE
    assert layout(L, mixed) == (DOUBLE, 3, 3, 0, 3, 1, 1)


# ---- errors ----------------------------------------------------------------------------------------------------

def test_errors(L):
    def err(r, status, *words):
        assert r[0] == status and r[1] == -1, (r, L.mpjx_last_error())
        msg = L.mpjx_last_error()
        for w in words:
            assert w in msg, (w, msg)
    err(struct(L, [1, 1], [0, 4], [INT, DOUBLE]), ERR_ARG, b"Base types of all component types in a Struct must agree")
    err(struct(L, [1, -2], [0, 4], [INT, INT]), ERR_ARG, b"-2", b"index 1")
    err(struct(L, [1, -2], [0, 4], [INT, UB]), ERR_ARG, b"-2")
    err(struct(L, [1, 1], [0, 4], [INT, 9]), ERR_ARG, b"datatype code 9", b"index 1")
    err(struct(L, [1, 1], [-1, 4], [INT, UB]), ERR_UNSUPPORTED, b"negative displacement", b"-1", b"index 0")
    err(struct(L, [1, 1, 1], [0, 9, 3], [INT, LB, UB]), ERR_UNSUPPORTED, b"extent -6", b"lb 9", b"ub 3")
    code = ctypes.c_int(-1)
    assert L.mpjx_type_struct(1, arr([1]), arr([0]), (ctypes.c_int * 1)(INT), None) == ERR_ARG
    assert L.mpjx_type_struct(-1, arr([1]), arr([0]), (ctypes.c_int * 1)(INT), ctypes.byref(code)) == ERR_ARG
    assert L.mpjx_type_struct(1, arr([1]), arr([0]), None, ctypes.byref(code)) == ERR_ARG
    assert L.mpjx_type_struct(1, None, arr([0]), (ctypes.c_int * 1)(INT), ctypes.byref(code)) == ERR_ARG


def test_a_marker_outside_struct_is_err_arg(L):
    code, x = ctypes.c_int(-1), ctypes.c_int64()
    tab = arr([0])
    for m in (LB, UB):
        assert L.mpjx_type_size(m) == 0
        assert L.mpjx_type_contiguous(2, m, ctypes.byref(code)) == ERR_ARG
        assert L.mpjx_type_vector(2, 1, 2, m, ctypes.byref(code)) == ERR_ARG
        assert L.mpjx_type_hvector(2, 1, 2, m, ctypes.byref(code)) == ERR_ARG
        assert L.mpjx_type_indexed(1, arr([1]), arr([0]), m, ctypes.byref(code)) == ERR_ARG
        assert L.mpjx_type_hindexed(1, arr([1]), arr([0]), m, ctypes.byref(code)) == ERR_ARG
        assert L.mpjx_type_info(m, None, None, None) == ERR_ARG
        assert L.mpjx_type_layout(m, None, None, None, None) == ERR_ARG
        assert L.mpjx_type_true_bounds(m, None, None) == ERR_ARG
        assert L.mpjx_type_free(m) == ERR_ARG
        assert L.mpjx_op_check(3, m) == ERR_ARG
        assert L.mpjx_pack_size(1, m, ctypes.byref(x)) == ERR_ARG
        assert L.mpjx_alltoallv_dt(None, None, tab, tab, m, None, tab, tab, m, None) == ERR_ARG
        assert L.mpjx_alltoallv(None, None, tab, tab, None, tab, tab, m, None) == ERR_ARG
        assert L.mpjx_allreduce_dt(None, None, None, 1, m, 3, 0, None) == ERR_ARG
        assert L.mpjx_allreduce(None, None, None, 1, m, 3, 0, None) == ERR_ARG


def test_pack_size_keeps_comm_pack_size(L):
    """Comm.Pack_size's formula on the Struct's size, not Struct.packedSize's accumulating byteSize."""
    s = made(struct(L, [2, 1, 1], [0, 5, 9], [INT, INT, UB]))
    h = one(L, "mpjx_type_hindexed", 2, arr([2, 1]), arr([0, 5]), INT)
    a, b = ctypes.c_int64(), ctypes.c_int64()
    for count in (0, 1, 3, 3):  # asking twice gives the same answer
        assert L.mpjx_pack_size(count, s, ctypes.byref(a)) == 0 and L.mpjx_pack_size(count, h, ctypes.byref(b)) == 0
        assert a.value == b.value


# ---- the mirrors -----------------------------------------------------------------------------------------------

def test_python_mirror():
    from mpjexpress_amd.mpi import MPI, Datatype, MPIException

    c4 = Datatype.Contiguous(4, MPI.INT)
    t = Datatype.Struct([2, 1, 1], [2, -3, 86], [c4, MPI.LB, MPI.UB])
    assert (t.Size(), t.Extent(), t.Lb(), t.Ub(), t.baseType, t.derived) == (8, 89, -3, 86, 5, True)
    t.Commit()
    col = Datatype.Struct([1, 1], [0, 1], [Datatype.Vector(5, 1, 8, MPI.DOUBLE), MPI.UB])
    assert (col.Size(), col.Extent(), col.Lb(), col.Ub(), col.true_ub, col.byteSize) == (5, 1, 0, 1, 33, 40)
    # Ub() is the library's, not lb + extent: the same here, but read from mpjx_type_layout
    pad = Datatype.Vector(2, 1, 2, Datatype.Struct([1, 1], [0, 3], [MPI.INT, MPI.UB]))
    assert (pad.Size(), pad.Extent(), pad.Lb(), pad.Ub()) == (2, 9, 0, 9)
    assert (MPI.LB.code, MPI.UB.code, MPI.LB.Size(), MPI.UB.Size()) == (10, 11, 0, 0)
    with pytest.raises(MPIException, match=r"\(-1\).*must agree"):
        Datatype.Struct([1, 1], [0, 2], [MPI.INT, MPI.FLOAT])
    with pytest.raises(MPIException, match=r"\(-1\)"):
        Datatype.Contiguous(2, MPI.UB)
    with pytest.raises(MPIException, match=r"\(-6\).*extent -6"):
        Datatype.Struct([1, 1, 1], [0, 9, 3], [MPI.INT, MPI.LB, MPI.UB])
    with pytest.raises(MPIException, match="2 block lengths, 1 displacements and 2 types"):
        Datatype.Struct([1, 1], [0], [MPI.INT, MPI.UB])
    for x in (t, col, pad, c4):
        x.Free()


CPP = r"""
#include <stdio.h>
#include "mpjx.hpp"
int main() {
  using mpi::Datatype; using mpi::MPI;
  Datatype c4 = Datatype::Contiguous(4, MPI::INT);
  Datatype t = Datatype::Struct({2, 1, 1}, {2, -3, 86}, {c4, MPI::LB, MPI::UB});
  if (t.Size() != 8 || t.Extent() != 89 || t.Lb() != -3 || t.Ub() != 86 || t.Base() != MPJX_INT) return 1;
  Datatype z = Datatype::Struct({1, 1}, {2, 2}, {MPI::INT, MPI::UB});  // extent 0 is an extent
  if (z.Size() != 1 || z.Extent() != 0 || z.Lb() != 2 || z.Ub() != 2) return 2;
  Datatype col = Datatype::Struct({1, 1}, {0, 1}, {Datatype::Vector(5, 1, 8, MPI::DOUBLE), MPI::UB});
  if (col.Size() != 5 || col.Extent() != 1 || col.Ub() != 1) return 3;
  if (MPI::INT.Extent() != 1 || MPI::DOUBLE2.Extent() != 2 || MPI::DOUBLE2.Ub() != 2) return 4;
  try {
    Datatype::Struct({1, 1}, {0, 2}, {MPI::INT, MPI::DOUBLE});
    return 5;
  } catch (const mpi::MPIException& e) {
    if (!strstr(e.what(), "must agree")) return 6;
  }
  try {
    Datatype::Contiguous(2, MPI::LB);
    return 7;
  } catch (const mpi::MPIException&) {
  }
  unsigned m = 7;
  if (mpjx_comm_last_move_kernels(nullptr, &m) != MPJX_ERR_ARG || m != 7) return 8;
  t.Free(); z.Free(); col.Free(); c4.Free();
  printf("struct_hpp: ok\n");
  return 0;
}
"""


def test_cpp_mirror(tmp_path):
    from mpjexpress_amd import _lib

    gxx = shutil.which("g++")
    assert gxx, "g++ is needed"
    src = tmp_path / "struct_hpp.cpp"
    src.write_text("#include <string.h>\n" + CPP)
    exe = str(tmp_path / "struct_hpp")
    libdir = os.path.dirname(_lib.LIB_PATH)
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        str(src), "-o", exe, "-L", libdir, "-lmpjx", f"-Wl,-rpath,{libdir}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "struct_hpp: ok" in r.stdout, (r.returncode, r.stdout, r.stderr[-2000:])


def test_header_and_exports(L):
    from mpjexpress_amd import _lib

    txt = open(HDR).read()
    assert "MPJX_LB = 10" in txt and "MPJX_UB = 11" in txt
    assert "int mpjx_type_struct(int n, const int64_t *blocklengths, const int64_t *displacements, const int *types," in txt
    assert "int mpjx_comm_last_move_kernels(mpjx_comm_t comm, unsigned *mask);" in txt
    assert "Struct.java:242-244" in txt  # where the reference departs from MPI's sticky rule
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for f in ("mpjx_type_struct", "mpjx_type_true_bounds", "mpjx_comm_last_move_kernels"):
        assert f in exported and f in _lib.EXPORTS, f
    m = ctypes.c_uint(7)
    assert L.mpjx_comm_last_move_kernels(None, ctypes.byref(m)) == ERR_ARG and m.value == 7


def test_no_device_is_needed():
    """A process that cannot see a GPU constructs, inspects and frees these types."""
    code = ("import ctypes\n"
            "from mpjexpress_amd import _lib\n"
            "L = _lib.lib()\n"
            "a = (ctypes.c_int64 * 2)(1, 1); d = (ctypes.c_int64 * 2)(0, 1); t = (ctypes.c_int * 2)(8, 11)\n"
            "c = ctypes.c_int(); e = ctypes.c_int64()\n"
            "assert L.mpjx_type_struct(2, a, d, t, ctypes.byref(c)) == 0\n"
            "assert L.mpjx_type_info(c.value, None, None, ctypes.byref(e)) == 0 and e.value == 1\n"
            "assert L.mpjx_type_free(c.value) == 0\n"
            "print('ok')\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1", PYTHONPATH=ROOT)
    r = subprocess.run([shutil.which("python3") or "python3", "-c", code], capture_output=True, text=True, env=env,
                       timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, r.stderr[-2000:]


def test_extent_zero_receive_is_err_arg(L):
    """Extent 0 with data is a type, and a send type; receiving more than one item of it is MPJX_ERR_ARG by the
    self-overlap rule. mpjx_unpack checks its arguments before it touches the communicator, so no device is needed:
    the pointers below are never dereferenced."""
    z = made(struct(L, [2, 1], [3, 3], [INT, UB]))
    assert layout(L, z) == (INT, 2, 0, 3, 3, 1, 0)
    ilv = made(struct(L, [3, 1], [0, 2], [INT, UB]))  # extent 2 under 3 elements: items share an element
    col = made(struct(L, [1, 1], [0, 1], [one(L, "mpjx_type_vector", 4, 1, 8, INT), UB]))  # interleaved, disjoint
    pos, st = ctypes.c_int64(0), ctypes.c_int(0)
    image, buf = ctypes.c_void_p(0x10000), ctypes.c_void_p(0x20000)

    def unpack(t, count):
        pos.value = 0
        rc = L.mpjx_unpack(None, image, 4096, ctypes.byref(pos), buf, count, t, ctypes.byref(st), None)
        return rc, L.mpjx_last_error()
    for t in (z, ilv):
        rc, msg = unpack(t, 2)
        assert rc == ERR_ARG and b"share a byte" in msg, msg
        rc, msg = unpack(t, 1)
        assert rc == ERR_ARG and b"comm is NULL" in msg, msg  # one item: every check passed
    rc, msg = unpack(col, 8)
    assert rc == ERR_ARG and b"comm is NULL" in msg, msg
    pos.value = 0  # packing FROM them is legal
    assert L.mpjx_pack(None, buf, 2, z, image, 4096, ctypes.byref(pos), None) == ERR_ARG
    assert b"comm is NULL" in L.mpjx_last_error()
