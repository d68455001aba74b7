"""Cases and expectations of the reductions on derived datatypes (mpjx_reduce_dt, mpjx_allreduce_dt,
mpjx_reduce_scatter_dt, mpjx_scan_dt and the mirrors' Reduce / Allreduce / Reduce_scatter / Scan with a derived
datatype), shared by tests/test_gpu_reduce_dt.py, tests/test_gpu_reduce_dt_matrix.py, the child-process worlds
and, on the CPU, tests/test_reduce_dt_case_power.py. All 13 types: BOOLEAN data is 0 / 1 bytes, CHAR unsigned 16
bits, a pair type two base elements per element (util.flat).

The expectation of every case:
  1. per rank, a send buffer filled over its WHOLE span by util.make_input / make_pair_input (specials
     included for FLOAT and DOUBLE), or by order_input below for the cases that pin an operand order;
  2. idx = form.index(count, off): the base-element indices of the type's blocks, in packed order (the forms
     of tests/strided_cases.py and tests/indexed_cases.py, described on their own, not through the library);
  3. the packed vectors send[idx] go through oracle.allreduce / reduce / reduce_scatter / scan with the call's
     flags;
  4. the expected receive buffer is the 0xA5 sentinel everywhere (in place: the send buffer's own bytes), with
     the oracle's result scattered to idx;
  5. the WHOLE buffer is compared byte for byte — util.same_bits' rule (any NaN equals any NaN for float SUM and
     PROD) on the data elements, the gaps raw;
  6. send buffers must come back unchanged unless the call is in place.

Below the helpers: the instantiation matrix (matrix_cases: every type of an op, both granule widths, one tile
and a partial one) and the order and root cases (order_group over ORDER_ROWS).
"""
import ctypes

import numpy as np

import indexed_cases as IC
import oracle as O
import strided_cases as SC
from mpjexpress_amd import _lib
from mpjexpress_amd.mpi import MPI
from util import flat, make_input

SENT = SC.SENT
TYPE_NAMES = ("BYTE", "CHAR", "SHORT", "BOOLEAN", "INT", "LONG", "FLOAT", "DOUBLE",
              "SHORT2", "INT2", "LONG2", "FLOAT2", "DOUBLE2")
ORACLE_TYPE = {name: getattr(O, name) for name in TYPE_NAMES}
for _name in TYPE_NAMES:
    SC.BASES.setdefault(_name, getattr(MPI, _name))  # the forms look their base type up there
FORM_CONTIGUOUS, FORM_MOVE, FORM_DIRECT, FORM_PACK = 1, 2, 3, 4
FLAG_OLD, FLAG_BLOCKING = 0x1, 0x10
K_FOLD, K_MST, K_SCAN = 0, 1, 2  # the kernel's kinds (mpjx_kernels.hpp)


class Case:
    """One collective call of a world of P ranks. `spec` is a type spec, or a function rank -> spec (ranks
    whose layouts differ); `n` the count, or Reduce_scatter's recvcounts; `inplace` the ranks whose receive
    buffer is their send buffer. `gen` = "order" fills the send buffers with order_input instead of
    util.make_input. `width` states which granule the call is built to take, "vec" (16 B) or "elem" (one
    element): run_rank asserts the host rule's preconditions on this rank's pointers and the layout."""

    def __init__(self, kind, base, spec, n, op, soff=0, roff=0, root=0, old=False, inplace=(), seed=1, gen=None,
                 width=None):
        self.kind, self.base, self.spec, self.n, self.op = kind, base, spec, n, op
        self.soff, self.roff, self.root, self.old, self.inplace, self.seed = soff, roff, root, old, set(inplace), seed
        self.gen, self.width = gen, width

    def __repr__(self):
        return (f"{self.kind} {self.base} {O.OP_NAMES[self.op]} {self.spec} x{self.n} @{self.soff}/{self.roff} "
                f"root {self.root}{' old' if self.old else ''}"
                f"{' in place ' + str(sorted(self.inplace)) if self.inplace else ''}")

    def form(self, r):
        return IC.form(self.base, self.spec(r) if callable(self.spec) else self.spec)

    def flags(self):
        return O.FLAG_OLD if self.old else 0

    def counts(self, P, r):
        """(items read from send, items written to recv) on rank r"""
        if self.kind == "reduce_scatter":
            return sum(self.n[:P]), self.n[r]
        return self.n, (self.n if self.kind != "reduce" or r == self.root else 0)


def nbytes(form, count, off):
    """A buffer that holds `count` items at base element `off`, three elements to spare, a multiple of 16 B"""
    return -(-((form.span(count, off) + 3) * form.bsz + 5) // 16) * 16


def order_input(type_, n, seed, op):
    """n elements of a float type, or pairs of a float pair type, made so that the ORDER of a combine shows in
    the result's bits (util.make_input's specials are too sparse for that: a quarter of the elements, one of
    twelve values each).
      MAX, MIN, MAXLOC, MINLOC  three values in four are NaN, +0 or -0, the rest +-1, +-inf or a small integer:
                                `x > y ? x : y` keeps a NaN accumulator and drops a NaN operand, and +0 == -0
                                compare equal with different bits, so which operand meets which first decides
                                most elements. The pairs' indices are spread over 0..999.
      SUM, PROD                 +-(1 + u) * 2^k, k uniform over 25 binades (SUM) or 13 (PROD): no two
                                associations of a sum round alike, and no product of 8 leaves the normal range."""
    rng = np.random.default_rng(seed)
    fd = O.NP_DTYPE[O.PAIR_BASE.get(type_, type_)]
    assert np.dtype(fd).kind == "f", "the order generator is for the float types"
    if op in (O.SUM, O.PROD):
        k = rng.integers(-12, 13, n) if op == O.SUM else rng.integers(-6, 7, n)
        v = np.ldexp((1.0 + rng.random(n)) * rng.choice([-1.0, 1.0], n), k).astype(fd)
    else:
        dense = np.array([np.nan, 0.0, -0.0], fd)
        rest = np.array([1.0, -1.0, np.inf, -np.inf, 2.0, -2.0, 3.0], fd)
        v = np.where(rng.random(n) < 0.75, dense[rng.integers(0, dense.size, n)], rest[rng.integers(0, rest.size, n)])
    if type_ not in O.PAIR_BASE:
        return v
    a = np.zeros(n, O.NP_DTYPE[type_])
    a["v"] = v
    a["l"] = rng.integers(0, 1000, n)
    return a


def inputs(case, P):
    """Per rank: the send buffer's bytes, and its packed vector in the oracle's dtype."""
    t = ORACLE_TYPE[case.base]
    per = 2 if t in O.PAIR_BASE else 1
    sends, packed = [], []
    for r in range(P):
        f = case.form(r)
        ns, _ = case.counts(P, r)
        nel = nbytes(f, ns, case.soff) // f.bsz
        seed = 7919 * case.seed + 31 * r + P
        if case.gen == "order":
            raw = flat(order_input(t, -(-nel // per), seed, case.op), t)[:nel]
        else:
            raw = flat(make_input(t, -(-nel // per), seed, op=case.op), t)[:nel]
        sends.append(np.ascontiguousarray(raw).view(np.uint8).copy())
        packed.append(raw[f.index(ns, case.soff)].copy().view(O.NP_DTYPE[t]))
    n0 = packed[0].size
    assert all(p.size == n0 for p in packed), "the case's packed lengths differ"
    return sends, packed


def combine(case, P, packed, root=None, old=None):
    """The oracle's packed result per rank (Reduce: significant at the root only) of `case` on the packed
    vectors; `root` and `old` replace the case's own (the mutations of tests/test_reduce_dt_case_power.py)."""
    t = ORACLE_TYPE[case.base]
    per = 2 if t in O.PAIR_BASE else 1
    root = case.root if root is None else root
    flags = O.FLAG_OLD if (case.old if old is None else old) else 0
    n0 = packed[0].size
    if n0 == 0:
        return [packed[r] for r in range(P)]
    if case.kind == "allreduce":
        return O.allreduce(packed, n0, t, case.op, flags=flags)
    if case.kind == "reduce":
        return O.reduce(packed, n0, t, case.op, root, flags=flags)
    if case.kind == "scan":
        return O.scan(packed, n0, t, case.op, flags=flags)
    epi = case.form(0).size // per
    return O.reduce_scatter(packed, [c * epi for c in case.n[:P]], t, case.op, flags=flags)[0]


def expected(case, P):
    """Per rank: (send bytes, expected receive bytes or None where recv is not significant, receive indices)."""
    t = ORACLE_TYPE[case.base]
    per = 2 if t in O.PAIR_BASE else 1
    sends, packed = inputs(case, P)
    res = combine(case, P, packed)
    out = []
    for r in range(P):
        f = case.form(r)
        _, nr = case.counts(P, r)
        if case.kind == "reduce" and r != case.root:
            out.append((sends[r], None, None))
            continue
        inplace = r in case.inplace
        roff = case.soff if inplace else case.roff
        idx = f.index(nr, roff)
        exp = sends[r].copy() if inplace else np.full(nbytes(f, nr, roff), SENT, np.uint8)
        ev = exp.view(SC.np_base(f))
        ev[idx] = flat(np.ascontiguousarray(res[r][: idx.size // per]), t).view(SC.np_base(f))
        out.append((sends[r], exp, idx))
    return out


def differs(case, got, exp, idx, form, what):
    """None, or what differs between the whole receive buffer and its expectation"""
    t = ORACLE_TYPE[case.base]
    got = got.copy()
    if t in (O.FLOAT, O.DOUBLE) and case.op in (O.SUM, O.PROD) and idx is not None and idx.size:
        fd = O.NP_DTYPE[t]
        g, e = got.view(fd), exp.view(fd)
        both = idx[np.isnan(g[idx]) & np.isnan(e[idx])]
        g[both] = e[both]
    return SC.differs(got, exp, what)


def last_form(comm):
    f = ctypes.c_int(-1)
    _lib.call("mpjx_comm_last_dt_form", comm.handle, ctypes.byref(f))
    return f.value


def elem_bytes(base):
    """Bytes of one element of the reduction: a base element, or a (value, index) pair"""
    return SC.BASES[base].byteSize


def check_width(case, f, ptrs):
    """The granule width a call takes is not observable through the ABI, so a case that is there for one width
    asserts the host rule's preconditions (reduce_dt_granule_log; tests/cpp/reduce_dt_plan_test.cpp holds the
    same layouts and pointer residues against the rule itself): "vec" needs every pointer of every rank and the
    layout's block, stride and extent bytes to be multiples of 16; "elem" needs an element narrower than 16 B
    and this rank's send pointer off a 16-B boundary."""
    lay = [f.blocklen * f.bsz, f.stride * f.bsz, f.extent * f.bsz]
    if case.width == "vec":
        assert all(v % 16 == 0 for v in ptrs + lay), ("not the 16-B form", case, ptrs, lay)
    else:
        assert case.width == "elem" and elem_bytes(case.base) < 16 and ptrs[0] % 16, ("not the element form", case, ptrs)


def run_rank(torch, comm, case, data, form_expected, lib_types, device=0):
    """Rank comm.Rank()'s call of `case` through the mirror; returns the list of what differs (empty: the whole
    receive buffer equals the expectation, the send buffer is unchanged unless in place, and the call took
    `form_expected`). `lib_types` caches this rank's library types per spec."""
    me, P = comm.Rank(), comm.Size()
    f = case.form(me)
    send, exp, idx = data[me]
    dev = torch.device("cuda", device)
    td = SC.torch_dtype(torch, f)
    key = (case.base, f.spec)
    if key not in lib_types:
        lib_types[key] = f.make()
    dt = lib_types[key]
    op = next(o for o in (MPI.MAX, MPI.MIN, MPI.SUM, MPI.PROD, MPI.LAND, MPI.BAND, MPI.LOR, MPI.BOR, MPI.LXOR, MPI.BXOR,
                          MPI.MAXLOC, MPI.MINLOC) if o.opCode == case.op)
    sbuf = torch.from_numpy(send).to(dev).view(td)
    inplace = me in case.inplace
    rbuf = sbuf if inplace else None
    if exp is not None and not inplace:
        rbuf = torch.full((exp.size,), SENT, dtype=torch.uint8, device=dev).view(td)
    roff = case.soff if inplace else case.roff
    if case.width:
        check_width(case, f, [sbuf.data_ptr() + case.soff * f.bsz] +
                    ([rbuf.data_ptr() + roff * f.bsz] if rbuf is not None else []))
    assert MPI.isOldSelected == case.old, "the driver sets MPI.isOldSelected for the whole world"
    if case.kind == "allreduce":
        comm.Allreduce(sbuf, case.soff, rbuf, roff, case.n, dt, op)
    elif case.kind == "reduce":
        comm.Reduce(sbuf, case.soff, rbuf, roff, case.n, dt, op, case.root)
    elif case.kind == "scan":
        comm.Scan(sbuf, case.soff, rbuf, roff, case.n, dt, op)
    else:
        comm.Reduce_scatter(sbuf, case.soff, rbuf, roff, list(case.n[:P]), dt, op)
    torch.cuda.synchronize(dev)
    what = f"{case.kind} {case.base} {f.spec} x{case.n} @{case.soff}/{roff} op {case.op} rank {me}/{P}"
    bad = []
    got_form = last_form(comm)
    if got_form != form_expected:
        bad.append(f"{what}: took form {got_form}, expected {form_expected}")
    if exp is not None:
        bad.append(differs(case, rbuf.view(torch.uint8).cpu().numpy(), exp, idx, f, what))
    if not inplace:
        bad.append(SC.differs(sbuf.view(torch.uint8).cpu().numpy(), send, what + " (send buffer)"))
    return [m for m in bad if m]


def child_cases(P):
    """Allreduce, Reduce, Reduce_scatter and Scan on one Vector type and one Indexed type: what the child-process
    worlds run (the RCCL stand-in, IPC), where the calls take the pack path."""
    rc = [(2, 0, 3, 1)[r % 4] for r in range(P)]
    out = []
    for i, (base, spec) in enumerate((("INT", ("V", 5, 3, 7)), ("DOUBLE", ("H", (2, 2, 2), (1, 11, 5))))):
        out += [Case("allreduce", base, spec, 3, O.SUM, soff=1, roff=2, seed=61 + 4 * i),
                Case("reduce", base, spec, 3, O.MAX, soff=1, roff=0, root=P - 1, seed=62 + 4 * i),
                Case("reduce_scatter", base, spec, rc, O.MIN, soff=2, roff=1, seed=63 + 4 * i),
                Case("scan", base, spec, 3, O.SUM, soff=0, roff=3, seed=64 + 4 * i)]
    return out


def run_cases(torch, comm, cases, form_expected):
    """Every case on this rank (every rank builds the whole seeded world); returns what differs."""
    types, bad = {}, []
    try:
        for case in cases:
            bad += run_rank(torch, comm, case, expected(case, comm.Size()), form_expected, types)
    finally:
        for t in types.values():
            t.Free()
    return bad


# ---- the instantiation matrix (tests/test_gpu_reduce_dt_matrix.py) ------------------------------------------------
# Every (functor, kind, P, W) that launch_functor_dt can return: per (P, op), every type valid for the op at both
# granule widths through three calls, each of which must take the direct form.
#   Allreduce, new collectives        K_MST at P >= 3, K_FOLD at P = 2
#   Reduce, old collectives, root P-1 K_FOLD in the FT order
#   Scan                              K_SCAN
# The layout is Vector(3, 32 B, 48 B) in elements of the type: 32-B blocks at a 48-B stride, a 128-B extent. At
# offsets 0 / 0 of fresh allocations it takes the 16-B form; at send offset 1 and receive offset 2 (base elements)
# the element form, for every type narrower than 16 B (LONG2 and DOUBLE2 are their own 16-B granule: one width).
# The count is the smallest that gives one full tile and a partial one: 256 lanes x DtUnroll<P, W> granules and
# a handful, so the `u` loop, the `q < nq` guard and the last partial tile all run and nothing more.
OPS = tuple(range(1, 13))
RI = ("H", (2, 2, 2), (1, 11, 5))   # lb = 1, blocks that go back and forth
SI = ("I", (3, 1, 2), (8, 0, 4))    # a displaced first block


def op_types(op):
    """The names of the types valid for `op`, in TYPE_NAMES' order"""
    return [n for n in TYPE_NAMES if O.check(op, ORACLE_TYPE[n]) == 0]


def dt_unroll(P, W):
    """DtUnroll<P, W> of mpjx_kernels_dt.hpp over Unroll<P> of mpjx_kernels.hpp"""
    return 1 if (W >= 8 and P >= 3) else (4 if P <= 2 else 2 if P <= 4 else 1)


def matrix_widths(base):
    """(width, W, soff, roff) of a type's matrix cases"""
    e = elem_bytes(base)
    return [("vec", 16 // e, 0, 0)] + ([("elem", 1, 1, 2)] if e < 16 else [])


def matrix_spec(base):
    e = elem_bytes(base)
    return ("V", 3, 32 // e, 48 // e)


def matrix_count(base, P, W):
    """Items of matrix_spec whose granules (W elements each) fill one tile of k_pway_dt and start a second"""
    per_item = 96 // (W * elem_bytes(base))
    return 256 * dt_unroll(P, W) // per_item + 1


def matrix_calls(P, base, spec, n, op, soff, roff, seed, width=None):
    """The three calls of the matrix on one layout: ([new-collectives cases], [old-collectives cases])"""
    return ([Case("allreduce", base, spec, n, op, soff=soff, roff=roff, seed=seed, width=width),
             Case("scan", base, spec, n, op, soff=soff, roff=roff, seed=seed + 1, width=width)],
            [Case("reduce", base, spec, n, op, soff=soff, roff=roff, root=P - 1, old=True, seed=seed + 2, width=width)])


def matrix_cases(P, op):
    """([new-collectives cases], [old-collectives cases]) of one matrix test"""
    new, old = [], []
    names = op_types(op)
    for i, base in enumerate(names):
        for j, (width, W, soff, roff) in enumerate(matrix_widths(base)):
            a, b = matrix_calls(P, base, matrix_spec(base), matrix_count(base, P, W), op, soff, roff,
                                1000 + 100 * op + 8 * i + 4 * j, width)
            new, old = new + a, old + b
    # one irregular layout: the table search of reduce_dt_offset, on a type that moves with P
    a, b = matrix_calls(P, names[P % len(names)], RI if P % 2 else SI, 3, op, 1, 2, 1000 + 100 * op + 96)
    return new + a, old + b


def matrix_launches(P, op):
    """The (op, type name, kind, P, W) of every k_pway_dt launch of matrix_cases' regular layouts"""
    out = []
    for base in op_types(op):
        for _, W, _, _ in matrix_widths(base):
            out += [(op, base, K_MST if P >= 3 else K_FOLD, P, W), (op, base, K_FOLD, P, W), (op, base, K_SCAN, P, W)]
    return out


# ---- order and root cases (tests/test_gpu_reduce_dt.py; their power: tests/test_reduce_dt_case_power.py) ----------
# Integer ops cannot show a wrong operand order or root, and float SUM hardly shows a root; float MAX / MIN and
# the float pair types show both on order_input's dense NaN and +-0, float SUM / PROD show the FT-vs-MST choice
# and the Scan order on its spread exponents. Every case runs on one 16-B-form layout and one element-form
# layout, 18 to 30 packed elements each.
ORDER_LAYOUTS = {  # base: ((spec, count, soff, roff, width) of the 16-B form, the same of the element form)
    "FLOAT": ((("V", 3, 8, 12), 1, 0, 0, "vec"), (("V", 5, 3, 7), 2, 1, 2, "elem")),
    "DOUBLE": ((("V", 3, 4, 6), 2, 0, 0, "vec"), (("V", 5, 3, 7), 2, 1, 2, "elem")),
    "FLOAT2": ((("V", 3, 4, 6), 2, 0, 0, "vec"), (("V", 5, 3, 7), 2, 2, 4, "elem")),  # whole pairs: offsets even
    "DOUBLE2": ((("V", 3, 2, 3), 3, 0, 0, "vec"), (("V", 5, 3, 7), 2, 2, 0, None)),    # a pair is its own granule
}


def ragged(P):
    return [(2, 0, 3, 1)[r % 4] for r in range(P)]


def rs_counts(P, k):
    """Reduce_scatter's recvcounts on layout k: ragged, with a zero. At P = 2 rank 1 always receives: its block is
    where the ring order {in[1], in[0]} differs from MST's and FT's {in[0], in[1]}."""
    return ([0, 3], [2, 1])[k] if P == 2 else ragged(P)


def order_group(row, P):
    """The cases of one row of the order table on a world of P ranks"""
    cases, seed = [], [100 * (1 + ORDER_ROWS.index((row, P)))]

    def add(kind, base, op, old=False, root=0, inplace=()):
        for k, (spec, n, soff, roff, width) in enumerate(ORDER_LAYOUTS[base]):
            seed[0] += 1
            cases.append(Case(kind, base, spec, rs_counts(P, k) if kind == "reduce_scatter" else n, op, soff=soff,
                              roff=roff, root=root, old=old, inplace=inplace, seed=seed[0], gen="order", width=width))
    if row == "reduce_max":
        for root in range(P):
            add("reduce", "FLOAT", O.MAX, root=root)
            add("reduce", "DOUBLE2", O.MAXLOC, root=root)
    elif row == "reduce_min":
        for root in range(P):
            add("reduce", "DOUBLE", O.MIN, root=root)
            add("reduce", "FLOAT2", O.MINLOC, root=root)
    elif row == "reduce_old":
        for root in (0, P - 1):
            add("reduce", "FLOAT", O.SUM, old=True, root=root)
            add("reduce", "FLOAT", O.MAX, old=True, root=root)
    elif row in ("reduce_scatter", "reduce_scatter_old"):
        for base, op in (("FLOAT", O.MAX), ("FLOAT", O.SUM), ("DOUBLE2", O.MAXLOC)):
            add("reduce_scatter", base, op, old=row.endswith("old"))
    elif row == "scan":
        for op in (O.SUM, O.PROD, O.MAX):
            add("scan", "FLOAT", op)
    else:
        assert row == "allreduce_old"
        add("allreduce", "FLOAT", O.SUM, old=True)
        add("allreduce", "FLOAT", O.SUM, old=True, inplace=[P - 1])
    return cases


ORDER_ROWS = ([("reduce_max", P) for P in (2, 3, 5, 8)] + [("reduce_min", P) for P in (4, 7)] +
              [("reduce_old", P) for P in (3, 6)] + [("reduce_scatter", P) for P in (2, 3, 5, 8)] +
              [("reduce_scatter_old", P) for P in (2, 3)] + [("scan", P) for P in (2, 3, 4, 8)] +
              [("allreduce_old", 4)])
