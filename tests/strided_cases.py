"""Cases and expectations of the strided block moves (mpjx_alltoallv_dt and the mirrors' calls with a derived
datatype), shared by tests/test_gpu_strided*.py, tests/strided_driver.py and tests/strided_ipc_worker.py.

As in tests/moves_cases.py no oracle is needed: a case is, per rank, a send buffer of seeded bytes, the call's
tables and the WHOLE receive buffer as it must look afterwards: a sentinel everywhere but inside the receive
layouts' blocks, which numpy indexing fills from the senders' buffers. Everything is compared as raw bytes,
so a write into a gap between two blocks fails like a wrong byte does.

A type is described here on its own, not through the library: ("V", count, blocklength, stride) or ("C", n)
over a basic or pair type name; `form` gives its blocks in base elements.
"""
import numpy as np

from mpjexpress_amd.mpi import MPI, Datatype

SENT = 0xA5
BASES = {"BYTE": MPI.BYTE, "CHAR": MPI.CHAR, "INT": MPI.INT, "DOUBLE": MPI.DOUBLE, "DOUBLE2": MPI.DOUBLE2}
METHODS = ("allgather", "allgatherv", "gatherv", "scatterv", "alltoall", "alltoallv", "gather", "scatter", "bcast")
ROOTED = ("gatherv", "scatterv", "gather", "scatter", "bcast")


class Form:
    """nblocks blocks of blocklen base elements, stride apart (all in base elements of `base`)."""

    def __init__(self, base, spec):
        self.base, self.spec = BASES[base], spec
        per = self.base.size  # 2 for a pair type
        if spec[0] == "V":
            _, c, b, s = spec
            self.nblocks, self.blocklen, self.stride = c, b * per, s * per
            if c == 0 or b == 0:
                self.nblocks = self.blocklen = self.stride = 0
        else:
            self.nblocks, self.blocklen, self.stride = (1, spec[1] * per, spec[1] * per) if spec[1] else (0, 0, 0)
        self.size = self.nblocks * self.blocklen
        self.extent = (self.nblocks - 1) * self.stride + self.blocklen if self.nblocks else 0
        self.bsz = self.base.baseSize

    def make(self):
        """The library's Datatype of this form."""
        if self.spec[0] == "V":
            return Datatype.Vector(self.spec[1], self.spec[2], self.spec[3], self.base)
        return Datatype.Contiguous(self.spec[1], self.base)

    def index(self, count, first):
        """Base-element indices of `count` items whose first element is `first`, in packed order."""
        k = np.arange(count, dtype=np.int64)[:, None, None] * self.extent
        b = np.arange(self.nblocks, dtype=np.int64)[None, :, None] * self.stride
        w = np.arange(self.blocklen, dtype=np.int64)[None, None, :]
        return (first + k + b + w).ravel()

    def span(self, count, first):
        return first + count * self.extent if count and self.size else 0


def np_base(form):
    return {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[form.bsz]


def torch_dtype(torch, form):
    return {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[form.bsz]


class Side:
    """One rank's send or receive side: a type, the Python offset (base elements) and per-peer (count, disp)."""

    def __init__(self, form, off, counts, displs):
        self.form, self.off, self.counts, self.displs = form, off, list(counts), list(displs)

    def elements(self):
        return max([self.form.span(c, self.off + d) for c, d in zip(self.counts, self.displs)] + [0])

    def nbytes(self):
        return -(-((self.elements() + 3) * self.form.bsz + 5) // 16) * 16

    def index(self, j):
        return self.form.index(self.counts[j], self.off + self.displs[j])


def fill(world, seed=0):
    """world = [(send Side, recv Side)] per rank. Returns per rank (send bytes, expected receive bytes)."""
    P = len(world)
    sends = [np.random.default_rng(7919 * seed + 31 * r + P).integers(0, 256, world[r][0].nbytes(), dtype=np.uint8)
             for r in range(P)]
    out = []
    for r in range(P):
        rs = world[r][1]
        exp = np.full(rs.nbytes(), SENT, np.uint8)
        ev = exp.view(np_base(rs.form))
        for i in range(P):
            ss = world[i][0]
            src = sends[i].view(np_base(ss.form))[ss.index(r)]
            dst = rs.index(i)
            assert src.size == dst.size, ("the case's packed lengths differ", i, r, src.size, dst.size)
            ev[dst] = src
        out.append((sends[r], exp))
    return out


def differs(got, exp, what):
    if np.array_equal(got, exp):
        return None
    bad = np.flatnonzero(got != exp)
    return f"{what}: {bad.size} bytes differ, first at byte {bad[0]} (got {got[bad[0]]:#x}, expected {exp[bad[0]]:#x})"


# ---- the nine mirror methods ------------------------------------------------------------------------------
SV, RV = ("V", 3, 2, 5), ("V", 2, 3, 4)  # 6 elements each, of different blocking
MODES = ("send", "recv", "both")


def ragged(i, j):
    """Items rank i sends to rank j."""
    return 0 if (7 * i + 3 * j) % 5 == 0 else 1 + ((13 * i + 7 * j) % 4)


def gaps(form, counts, salt=0):
    """Displacements in base elements with gaps, descending in rank order."""
    d, pos = [0] * len(counts), 1 + salt
    for j in reversed(range(len(counts))):
        d[j] = pos
        pos += counts[j] * form.extent + 1 + (j + salt) % 3
    return d


def mode_forms(base, mode, per=6):
    """(send form, recv form, items -> send count, items -> recv count) of a mode: a Vector on the send side,
    on the receive side, or on both; the other side is the plain base type."""
    plain = Form(base, ("C", 1))
    if mode == "send":
        return Form(base, SV), plain, (lambda n: n), (lambda n: n * per)
    if mode == "recv":
        return plain, Form(base, RV), (lambda n: n * per), (lambda n: n)
    return Form(base, SV), Form(base, RV), (lambda n: n), (lambda n: n)


def method_world(method, P, base, mode, root=0, soff=1, roff=2):
    """[(send Side, recv Side)] per rank, as the MPI rules of `method` lay the messages out: block j of an
    equal-count call starts j * count extents into the buffer, the v-calls' displacements are base elements."""
    sf, rf, sn, rn = mode_forms(base, mode)
    if method in ("gather", "scatter", "bcast"):  # one datatype argument: the same Vector on both sides
        sf = rf = Form(base, RV if mode == "recv" else SV)
        sn = rn = lambda n: n  # noqa: E731
    z = [0] * P
    n = 2
    M = [[ragged(i, j) for j in range(P)] for i in range(P)]
    own = [ragged(j, 2 * j + 1) for j in range(P)]
    world = []
    for r in range(P):
        at = lambda v: [v if j == root else 0 for j in range(P)]  # noqa: E731
        if method == "allgather":
            s = Side(sf, soff, [sn(n)] * P, z)
            q = Side(rf, roff, [rn(n)] * P, [j * rn(n) * rf.extent for j in range(P)])
        elif method == "allgatherv":
            s = Side(sf, soff, [sn(own[r])] * P, z)
            rc = [rn(c) for c in own]
            q = Side(rf, roff, rc, gaps(rf, rc))
        elif method == "gatherv":
            s = Side(sf, soff, at(sn(M[r][root])), z)
            rc = [rn(M[j][root]) for j in range(P)] if r == root else z
            q = Side(rf, roff, rc, gaps(rf, rc) if r == root else z)
        elif method == "scatterv":
            sc = [sn(c) for c in M[root]] if r == root else z
            s = Side(sf, soff, sc, gaps(sf, sc) if r == root else z)
            q = Side(rf, roff, at(rn(M[root][r])), z)
        elif method == "alltoall":
            s = Side(sf, soff, [sn(n)] * P, [j * sn(n) * sf.extent for j in range(P)])
            q = Side(rf, roff, [rn(n)] * P, [j * rn(n) * rf.extent for j in range(P)])
        elif method == "alltoallv":
            sc, rc = [sn(c) for c in M[r]], [rn(M[j][r]) for j in range(P)]
            s, q = Side(sf, soff, sc, gaps(sf, sc)), Side(rf, roff, rc, gaps(rf, rc, 1))
        elif method == "gather":
            s = Side(sf, soff, at(sn(n)), z)
            q = Side(rf, roff, [rn(n)] * P if r == root else z, [j * rn(n) * rf.extent for j in range(P)] if r == root else z)
        elif method == "scatter":
            s = Side(sf, soff, [sn(n)] * P if r == root else z, [j * sn(n) * sf.extent for j in range(P)] if r == root else z)
            q = Side(rf, roff, at(rn(n)), z)
        elif method == "bcast":  # the root keeps its own bytes: nothing is received there
            s = Side(sf, soff, [0 if j == root else sn(n) for j in range(P)] if r == root else z, z)
            q = Side(rf, soff, at(rn(n)) if r != root else z, z)
        else:
            raise ValueError(method)
        world.append((s, q))
    return world


def method_call(comm, method, s, q, st, rt, sbuf, rbuf, root):
    """The mpiJava call of rank sides (s, q) with library types st, rt on device tensors."""
    me, P = comm.Rank(), comm.Size()
    if method == "allgather":
        comm.Allgather(sbuf, s.off, s.counts[0], st, rbuf, q.off, q.counts[0], rt)
    elif method == "allgatherv":
        comm.Allgatherv(sbuf, s.off, s.counts[0], st, rbuf, q.off, q.counts, q.displs, rt)
    elif method == "gatherv":
        comm.Gatherv(sbuf, s.off, s.counts[root], st, rbuf, q.off, q.counts, q.displs, rt, root)
    elif method == "scatterv":
        comm.Scatterv(sbuf, s.off, s.counts, s.displs, st, rbuf, q.off, q.counts[root], rt, root)
    elif method == "alltoall":
        comm.Alltoall(sbuf, s.off, s.counts[0], st, rbuf, q.off, q.counts[0], rt)
    elif method == "alltoallv":
        comm.Alltoallv(sbuf, s.off, s.counts, s.displs, st, rbuf, q.off, q.counts, q.displs, rt)
    elif method == "gather":
        comm.Gather(sbuf, s.off, s.counts[root], rbuf, q.off, s.counts[root], st, root)
    elif method == "scatter":
        comm.Scatter(sbuf, s.off, q.counts[root], rbuf, q.off, q.counts[root], st, root)
    else:  # bcast: one buffer; the root's is the send buffer, every other rank's the receive buffer
        n = s.counts[(root + 1) % P] if me == root else q.counts[root]
        comm.Bcast(sbuf if me == root else rbuf, s.off, n if P > 1 else 0, st, root)


def matrix(P):
    """(method, mode, root) for all nine methods, a Vector on the send side, the receive side and both; rooted
    calls at roots 0 and P - 1."""
    out = []
    for method in METHODS:
        for mode in MODES:
            for root in ((0, P - 1) if method in ROOTED and P > 1 else (0,)):
                out.append((method, mode, root))
    return out


def run_methods(torch, comm, P, base, todo, types, device=0):
    """Run every (method, mode, root) of `todo` on this rank; returns the list of differences (empty: all the
    receive buffers equal the expectation byte for byte and no send buffer changed). `types` caches the
    library types per form spec for this rank."""
    me, bad = comm.Rank(), []
    dev = torch.device("cuda", device)

    def lib_type(form):
        key = (form.base.name, form.spec)
        if key not in types:
            types[key] = form.base if form.spec == ("C", 1) else form.make()
        return types[key]
    for method, mode, root in todo:
        world = method_world(method, P, base, mode, root)
        send, exp = fill(world, seed=len(method) + 3 * MODES.index(mode) + root)[me]
        s, q = world[me]
        td = torch_dtype(torch, s.form)
        sbuf = torch.from_numpy(send).to(dev).view(td)
        rbuf = torch.full((exp.size,), SENT, dtype=torch.uint8, device=dev).view(td)
        method_call(comm, method, s, q, lib_type(s.form), lib_type(q.form), sbuf, rbuf, root)
        torch.cuda.synchronize(dev)
        what = f"{method} {mode} root {root} rank {me}/{P}"
        bad.append(differs(rbuf.view(torch.uint8).cpu().numpy(), exp, what))
        bad.append(differs(sbuf.view(torch.uint8).cpu().numpy(), send, what + " (send buffer)"))
    return [m for m in bad if m]
