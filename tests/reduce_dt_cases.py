"""Cases and expectations of the reductions on derived datatypes (mpjx_reduce_dt, mpjx_allreduce_dt,
mpjx_reduce_scatter_dt, mpjx_scan_dt and the mirrors' Reduce / Allreduce / Reduce_scatter / Scan with a derived
datatype), shared by tests/test_gpu_reduce_dt.py and the C-ABI tests.

The expectation of every case:
  1. per rank, a send buffer filled over its WHOLE span by util.make_input / make_pair_input (specials
     included for FLOAT and DOUBLE);
  2. idx = form.index(count, off): the base-element indices of the type's blocks, in packed order (the forms
     of tests/strided_cases.py and tests/indexed_cases.py, described on their own, not through the library);
  3. the packed vectors send[idx] go through oracle.allreduce / reduce / reduce_scatter / scan with the call's
     flags;
  4. the expected receive buffer is the 0xA5 sentinel everywhere (in place: the send buffer's own bytes), with
     the oracle's result scattered to idx;
  5. the WHOLE buffer is compared byte for byte — util.same_bits' rule (any NaN equals any NaN for float SUM and
     PROD) on the data elements, the gaps raw;
  6. send buffers must come back unchanged unless the call is in place.
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
SC.BASES.setdefault("FLOAT", MPI.FLOAT)  # the forms look their base type up there
SC.BASES.setdefault("LONG", MPI.LONG)
ORACLE_TYPE = {"BYTE": O.BYTE, "CHAR": O.CHAR, "INT": O.INT, "LONG": O.LONG, "FLOAT": O.FLOAT, "DOUBLE": O.DOUBLE,
               "DOUBLE2": O.DOUBLE2}
FORM_CONTIGUOUS, FORM_MOVE, FORM_DIRECT, FORM_PACK = 1, 2, 3, 4
FLAG_OLD, FLAG_BLOCKING = 0x1, 0x10


class Case:
    """One collective call of a world of P ranks. `spec` is a type spec, or a function rank -> spec (ranks
    whose layouts differ); `n` the count, or Reduce_scatter's recvcounts; `inplace` the ranks whose receive
    buffer is their send buffer."""

    def __init__(self, kind, base, spec, n, op, soff=0, roff=0, root=0, old=False, inplace=(), seed=1):
        self.kind, self.base, self.spec, self.n, self.op = kind, base, spec, n, op
        self.soff, self.roff, self.root, self.old, self.inplace, self.seed = soff, roff, root, old, set(inplace), seed

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


def expected(case, P):
    """Per rank: (send bytes, expected receive bytes or None where recv is not significant, receive indices)."""
    t = ORACLE_TYPE[case.base]
    per = 2 if t in O.PAIR_BASE else 1
    sends, packed = [], []
    for r in range(P):
        f = case.form(r)
        ns, _ = case.counts(P, r)
        nel = nbytes(f, ns, case.soff) // f.bsz
        raw = flat(make_input(t, -(-nel // per), 7919 * case.seed + 31 * r + P, op=case.op), t)[:nel]
        sends.append(np.ascontiguousarray(raw).view(np.uint8).copy())
        packed.append(raw[f.index(ns, case.soff)].copy().view(O.NP_DTYPE[t]))
    n0 = packed[0].size
    assert all(p.size == n0 for p in packed), "the case's packed lengths differ"
    if n0 == 0:
        res = [packed[r] for r in range(P)]
    elif case.kind == "allreduce":
        res = O.allreduce(packed, n0, t, case.op, flags=case.flags())
    elif case.kind == "reduce":
        res = O.reduce(packed, n0, t, case.op, case.root, flags=case.flags())
    elif case.kind == "scan":
        res = O.scan(packed, n0, t, case.op, flags=case.flags())
    else:
        epi = case.form(0).size // per
        res, _ = O.reduce_scatter(packed, [c * epi for c in case.n[:P]], t, case.op, flags=case.flags())
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
