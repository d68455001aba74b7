"""Cases and expectations of the block moves with an irregular datatype (Hvector, Indexed, Hindexed), shared by
tests/test_gpu_indexed*.py, tests/indexed_driver.py and tests/indexed_ipc_worker.py.

The scheme is tests/strided_cases.py's (whose Side, fill, differs and method_call run unchanged over the
forms here): seeded send bytes, sentinel-filled receive buffers, the WHOLE receive buffer compared byte for
byte against numpy indexing. A type is described here on its own, not through the library, by the rules of
src/mpi/Indexed.java and src/mpi/Vector.java:
  ("I", blocklengths, displacements)        Indexed over the base type: block i starts disp[i] * old.extent
  ("H", blocklengths, displacements)        Hindexed: block i starts disp[i] BASE elements from the origin
  ("HV", count, bl, stride, (c, b, s))      Hvector of Vector(c, b, s, base): block j starts j * stride base
                                            elements from the origin
Blocks are packed in the arrays' order; lb / ub are the lowest element and one past the highest; the extent is
ub - lb; item k starts k * extent after the origin and lb is NOT subtracted.
"""
import numpy as np

import strided_cases as SC
from mpjexpress_amd.mpi import Datatype

SENT = SC.SENT
PLAIN = ("C", 1)


class IForm:
    """The blocks (offset, length) of one item in base elements, in pack order, zero-length ones dropped."""

    def __init__(self, base, spec):
        self.base, self.spec = SC.BASES[base], spec
        per = self.base.size  # 2 for a pair type: the old type's size and extent
        self.bsz = self.base.baseSize
        blocks = []
        if spec[0] in ("I", "H"):
            for bl, d in zip(spec[1], spec[2]):
                blocks.append((d * per if spec[0] == "I" else d, bl * per))
        else:
            _, count, bl, stride, (vc, vb, vs) = spec
            vext = ((vc - 1) * vs + vb) * per
            for j in range(count):
                for i in range(bl):
                    for c in range(vc):
                        blocks.append((j * stride + i * vext + c * vs * per, vb * per))
        self.blocks = [(o, n) for o, n in blocks if n > 0]
        self.size = sum(n for _, n in self.blocks)
        self.lb = min([o for o, _ in self.blocks] or [0])
        self.ub = max([o + n for o, n in self.blocks] or [0])
        self.extent = self.ub - self.lb
        self.item = np.concatenate([o + np.arange(n, dtype=np.int64) for o, n in self.blocks] or
                                   [np.zeros(0, np.int64)])

    def make(self):
        s = self.spec
        if s[0] == "I":
            return Datatype.Indexed(s[1], s[2], self.base)
        if s[0] == "H":
            return Datatype.Hindexed(s[1], s[2], self.base)
        v = Datatype.Vector(*s[4], self.base)
        try:
            return Datatype.Hvector(s[1], s[2], s[3], v)
        finally:
            v.Free()

    def index(self, count, first):
        k = np.arange(count, dtype=np.int64)[:, None] * self.extent
        return (first + k + self.item[None, :]).ravel()

    def span(self, count, first):
        return first + (count - 1) * self.extent + self.ub if count and self.size else 0


def form(base, spec):
    return SC.Form(base, spec) if spec[0] in ("V", "C") else IForm(base, spec)


def lib_type(f):
    return f.base if f.spec == PLAIN else f.make()


# ---- the nine mirror methods ------------------------------------------------------------------------------
# 6 elements each, of different blocking, both with displacements that go back and forth; RI has lb = 1
SI, RI = ("I", (3, 1, 2), (8, 0, 4)), ("H", (2, 2, 2), (1, 11, 5))
matrix = SC.matrix


def mode_forms(base, mode, per=6):
    plain = SC.Form(base, PLAIN)
    if mode == "send":
        return IForm(base, SI), plain, (lambda n: n), (lambda n: n * per)
    if mode == "recv":
        return plain, IForm(base, RI), (lambda n: n * per), (lambda n: n)
    return IForm(base, SI), IForm(base, RI), (lambda n: n), (lambda n: n)


def method_world(method, P, base, mode, root=0, soff=1, roff=2):
    """[(send Side, recv Side)] per rank, laid out as tests/strided_cases.py's method_world lays them out, with
    an irregular type where that has a Vector."""
    Side, gaps, ragged = SC.Side, SC.gaps, SC.ragged
    sf, rf, sn, rn = mode_forms(base, mode)
    if method in ("gather", "scatter", "bcast"):  # one datatype argument
        sf = rf = IForm(base, RI if mode == "recv" else SI)
        sn = rn = lambda n: n  # noqa: E731
    z, n = [0] * P, 2
    M = [[ragged(i, j) for j in range(P)] for i in range(P)]
    own = [ragged(j, 2 * j + 1) for j in range(P)]
    eq = lambda f, c: [j * c * f.extent for j in range(P)]  # noqa: E731  equal-count calls step by count * extent
    world = []
    for r in range(P):
        at = lambda v: [v if j == root else 0 for j in range(P)]  # noqa: E731
        if method == "allgather":
            s, q = Side(sf, soff, [sn(n)] * P, z), Side(rf, roff, [rn(n)] * P, eq(rf, rn(n)))
        elif method == "allgatherv":
            rc = [rn(c) for c in own]
            s, q = Side(sf, soff, [sn(own[r])] * P, z), Side(rf, roff, rc, gaps(rf, rc))
        elif method == "gatherv":
            rc = [rn(M[j][root]) for j in range(P)] if r == root else z
            s, q = Side(sf, soff, at(sn(M[r][root])), z), Side(rf, roff, rc, gaps(rf, rc) if r == root else z)
        elif method == "scatterv":
            sc = [sn(c) for c in M[root]] if r == root else z
            s, q = Side(sf, soff, sc, gaps(sf, sc) if r == root else z), Side(rf, roff, at(rn(M[root][r])), z)
        elif method == "alltoall":
            s, q = Side(sf, soff, [sn(n)] * P, eq(sf, sn(n))), Side(rf, roff, [rn(n)] * P, eq(rf, rn(n)))
        elif method == "alltoallv":
            sc, rc = [sn(c) for c in M[r]], [rn(M[j][r]) for j in range(P)]
            s, q = Side(sf, soff, sc, gaps(sf, sc)), Side(rf, roff, rc, gaps(rf, rc, 1))
        elif method == "gather":
            s = Side(sf, soff, at(sn(n)), z)
            q = Side(rf, roff, [rn(n)] * P if r == root else z, eq(rf, rn(n)) if r == root else z)
        elif method == "scatter":
            s = Side(sf, soff, [sn(n)] * P if r == root else z, eq(sf, sn(n)) if r == root else z)
            q = Side(rf, roff, at(rn(n)), z)
        elif method == "bcast":  # the root keeps its own bytes: nothing is received there
            s = Side(sf, soff, [0 if j == root else sn(n) for j in range(P)] if r == root else z, z)
            q = Side(rf, soff, at(rn(n)) if r != root else z, z)
        else:
            raise ValueError(method)
        world.append((s, q))
    return world


def run_methods(torch, comm, P, base, todo, types, device=0):
    """As tests/strided_cases.py's run_methods, over method_world above."""
    me, bad = comm.Rank(), []
    dev = torch.device("cuda", device)

    def cached(f):
        key = (f.base.name, f.spec)
        if key not in types:
            types[key] = lib_type(f)
        return types[key]
    for method, mode, root in todo:
        world = method_world(method, P, base, mode, root)
        send, exp = SC.fill(world, seed=len(method) + 3 * SC.MODES.index(mode) + root)[me]
        s, q = world[me]
        td = SC.torch_dtype(torch, s.form)
        sbuf = torch.from_numpy(send).to(dev).view(td)
        rbuf = torch.full((exp.size,), SENT, dtype=torch.uint8, device=dev).view(td)
        SC.method_call(comm, method, s, q, cached(s.form), cached(q.form), sbuf, rbuf, root)
        torch.cuda.synchronize(dev)
        what = f"{method} {mode} root {root} rank {me}/{P}"
        bad.append(SC.differs(rbuf.view(torch.uint8).cpu().numpy(), exp, what))
        bad.append(SC.differs(sbuf.view(torch.uint8).cpu().numpy(), send, what + " (send buffer)"))
    return [m for m in bad if m]
