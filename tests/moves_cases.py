"""Cases and expectations of the block-move collectives (Allgather(v), Gatherv, Scatterv, Alltoall(v)),
shared by tests/test_gpu_moves*.py, tests/moves_driver.py and tests/moves_ipc_worker.py.

Data movement needs no oracle: a case is, per rank, a send buffer of seeded bytes, the call's count and
displacement tables, and the WHOLE receive buffer as it must look afterwards — a sentinel everywhere but
the segments, which numpy slices out of the senders' buffers. Everything is compared as raw bytes, so a
stray write into a gap, or before or after a segment, fails like a wrong byte does.
"""
import json
import os

import numpy as np

from mpjexpress_amd.mpi import MPI

SENT = 0xA5
COLLS = ("allgather", "allgatherv", "gatherv", "scatterv", "alltoall", "alltoallv")
ROOTED = ("gatherv", "scatterv")
TYPES = {"BYTE": MPI.BYTE, "CHAR": MPI.CHAR, "INT": MPI.INT, "DOUBLE": MPI.DOUBLE, "DOUBLE2": MPI.DOUBLE2}
# Python offsets in base elements: nonzero and no multiple of 16 B (3, 6, 4, 8, 8 bytes)
OFFS = {"BYTE": 3, "CHAR": 3, "INT": 1, "DOUBLE": 1, "DOUBLE2": 1}
EQ = 37  # the equal-count calls' count
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ccl_moves_kat.json")


def ragged(i, j):
    """Elements rank i sends to rank j."""
    return 0 if (7 * i + 3 * j) % 5 == 0 else 1 + ((131 * i + 71 * j) % 97)


def layout(counts, salt=0):
    """Displacements (elements) with gaps, descending in rank order: the last rank's segment comes first."""
    d, pos = [0] * len(counts), 1 + salt
    for j in reversed(range(len(counts))):
        d[j] = pos
        pos += counts[j] + 1 + (j + salt) % 3
    return d


class Rank:
    """One rank's part of a case: tables in elements, buffers as bytes."""

    def __init__(self, dt, off, sc, sd, rc, rd, seed):
        self.dt, self.off = dt, off
        self.sc, self.sd, self.rc, self.rd = list(sc), list(sd), list(rc), list(rd)
        esz, offb = dt.byteSize, off * dt.baseSize
        self.offb = offb

        def size(c, d):
            span = max([dj + cj for cj, dj in zip(c, d) if cj > 0] or [0])
            return -(-(offb + (span + 2) * esz + 5) // 16) * 16
        self.send = np.random.default_rng(seed).integers(0, 256, size(sc, sd), dtype=np.uint8)
        self.nrecv = size(rc, rd)
        self.expect = None

    def sbytes(self, j):
        """The bytes this rank sends to rank j."""
        esz = self.dt.byteSize
        a = self.offb + self.sd[j] * esz
        return self.send[a:a + self.sc[j] * esz]


def make_case(coll, P, tname, root=0, seed=0, count=ragged, eq=EQ, off=None):
    """Per-rank Rank objects with .expect filled in."""
    dt = TYPES[tname]
    off = OFFS[tname] if off is None else off
    M = [[count(i, j) for j in range(P)] for i in range(P)]
    own = [count(j, 2 * j) for j in range(P)]  # Allgatherv: what rank j contributes (nothing at j % 5 == 0)
    zeros = [0] * P
    ranks = []
    for r in range(P):
        if coll == "alltoallv":
            sc, rc = M[r], [M[j][r] for j in range(P)]
            sd, rd = layout(sc), layout(rc, 1)
        elif coll == "alltoall":
            sc = rc = [eq] * P
            sd = rd = [j * eq for j in range(P)]
        elif coll == "allgather":
            sc, sd = [eq] * P, zeros
            rc, rd = [eq] * P, [j * eq for j in range(P)]
        elif coll == "allgatherv":
            sc, sd = [own[r]] * P, zeros
            rc, rd = own, layout(own)
        elif coll == "gatherv":
            sc, sd = [M[r][root] if j == root else 0 for j in range(P)], zeros
            rc = [M[j][root] for j in range(P)] if r == root else zeros
            rd = layout(rc) if r == root else zeros
        elif coll == "scatterv":
            sc = M[root] if r == root else zeros
            sd = layout(sc) if r == root else zeros
            rc, rd = [M[root][r] if j == root else 0 for j in range(P)], zeros
        else:
            raise ValueError(coll)
        ranks.append(Rank(dt, off, sc, sd, rc, rd, 1000003 * seed + 7919 * P + 31 * r + len(coll) + dt.code))
    esz = dt.byteSize
    for r, k in enumerate(ranks):
        e = np.full(k.nrecv, SENT, np.uint8)
        for j in range(P):
            b = ranks[j].sbytes(r)
            assert b.size == k.rc[j] * esz, (coll, r, j)
            a = k.offb + k.rd[j] * esz
            e[a:a + b.size] = b
        k.expect = e
    return ranks


def torch_dtype(torch, dt):
    return {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[dt.baseSize]


def call(comm, coll, k, s, r, root=0):
    """The mpiJava call of rank part k on device tensors s (send) and r (receive)."""
    dt, off, me = k.dt, k.off, comm.Rank()
    if coll == "allgather":
        comm.Allgather(s, off, k.sc[0], dt, r, off, k.rc[0], dt)
    elif coll == "allgatherv":
        comm.Allgatherv(s, off, k.sc[0], dt, r, off, k.rc, k.rd, dt)
    elif coll == "gatherv":
        comm.Gatherv(s, off, k.sc[root], dt, r, off, k.rc, k.rd, dt, root)
    elif coll == "scatterv":
        comm.Scatterv(s, off, k.sc, k.sd, dt, r, off, k.rc[root], dt, root)
    elif coll == "alltoall":
        comm.Alltoall(s, off, k.sc[me], dt, r, off, k.rc[me], dt)
    else:
        comm.Alltoallv(s, off, k.sc, k.sd, dt, r, off, k.rc, k.rd, dt)


def run_rank(torch, comm, coll, k, root=0, device=0):
    """Run rank part k; returns a message, or None if the receive buffer is the expectation byte for byte
    and the send buffer is unchanged."""
    dev = torch.device("cuda", device)
    td = torch_dtype(torch, k.dt)
    s = torch.from_numpy(k.send).to(dev).view(td)
    r = torch.full((k.nrecv,), SENT, dtype=torch.uint8, device=dev).view(td)
    call(comm, coll, k, s, r, root)
    torch.cuda.synchronize(dev)
    got = r.view(torch.uint8).cpu().numpy()
    if not np.array_equal(got, k.expect):
        bad = np.flatnonzero(got != k.expect)
        return (f"{coll} {k.dt} rank {comm.Rank()}/{comm.Size()}: {bad.size} bytes differ, first at byte {bad[0]} "
                f"(got {got[bad[0]]:#x}, expected {k.expect[bad[0]]:#x}; offset bytes {k.offb}, rc {k.rc}, rd {k.rd})")
    if not np.array_equal(s.view(torch.uint8).cpu().numpy(), k.send):
        return f"{coll} {k.dt} rank {comm.Rank()}: the send buffer changed"
    return None


def matrix(Ps, tnames):
    """(coll, P, type name, root) of the ragged six-collective matrix: rooted calls at roots 0 and P - 1."""
    out = []
    for P in Ps:
        for t in tnames:
            for coll in COLLS:
                for root in ((0, P - 1) if coll in ROOTED and P > 1 else (0,)):
                    out.append((coll, P, t, root))
    return out


# ---- the reference programs' known answers (tests/golden/ccl_moves_kat.json) ---------------------------
def kat():
    with open(GOLDEN) as f:
        return json.load(f)


def kat_cases(P):
    """[(name, coll, root, per-rank (send int32 array, sc, sd, rc, rd, receive length), per-rank expected
    int32 receive array)] of the six reference programs at P tasks; receive buffers start as zeros. The
    expectations come from the programs' statements by numpy indexing; at 3 tasks the tables the
    programs hold (`ans`) must equal them, which test_gpu_moves checks."""
    stride = 15
    cases = []
    # alltoallv.java
    ranks, exp = [], []
    for me in range(P):
        out = np.array([i + me * stride for _ in range(P) for i in range(stride)], np.int32)
        sc = [10 if me == 0 else 15] * P
        rc = [10] + [15] * (P - 1)
        ranks.append((out, sc, [j * stride for j in range(P)], rc, [j * 15 for j in range(P)], P * stride))
    for me in range(P):
        e = np.zeros(P * stride, np.int32)
        for j in range(P):
            n = ranks[me][3][j]
            e[j * 15:j * 15 + n] = ranks[j][0][me * stride:me * stride + n]
        exp.append(e)
    cases.append(("alltoallv", "alltoallv", 0, ranks, exp))
    # allgatherv.java / gatherv.java (root 0)
    for name, fill in (("allgatherv", lambda i: i), ("gatherv", lambda i: 1)):
        ranks, exp = [], []
        rc = [10] + [5] * (P - 1)
        dis = [j * stride for j in range(P)]
        for me in range(P):
            out = np.array([fill(i) for i in range(10)], np.int32)
            ranks.append((out, [rc[me]] * P, [0] * P, rc, dis, 10 * stride * P))
        for me in range(P):
            e = np.zeros(10 * stride * P, np.int32)
            if name == "allgatherv" or me == 0:
                for j in range(P):
                    e[dis[j]:dis[j] + rc[j]] = ranks[j][0][:rc[j]]
            exp.append(e)
        cases.append((name, name, 0, ranks, exp))
    # scatterv.java (root 0): in[k] = out[dis[rank] + k]
    scn = [10] + [5] * (P - 1)
    dis = [j * stride for j in range(P)]
    ranks = [(np.arange(P * stride, dtype=np.int32), scn, dis, [scn[me]] * P, [0] * P, 10) for me in range(P)]
    exp = [np.concatenate([np.arange(dis[me], dis[me] + scn[me], dtype=np.int32),
                           np.zeros(10 - scn[me], np.int32)]) for me in range(P)]
    cases.append(("scatterv", "scatterv", 0, ranks, exp))
    # allgather.java / alltoall.java: out[i] = rank, in[k + i*count] = i (count 10000 left to the sweep
    # tests: the same path as 1000)
    for name in ("allgather", "alltoall"):
        for n in (1, 10, 100, 1000):
            m = n * (P if name == "alltoall" else 1)
            ranks = [(np.full(m, me, np.int32), [n] * P, [0] * P, [n] * P, [0] * P, n * P) for me in range(P)]
            exp = [np.repeat(np.arange(P, dtype=np.int32), n) for _ in range(P)]
            cases.append((f"{name}_{n}", name, 0, ranks, exp))
    return cases


def kat_call(comm, coll, part, s, r, root):
    out, sc, sd, rc, rd, _ = part
    me = comm.Rank()
    if coll == "alltoallv":
        comm.Alltoallv(s, 0, sc, sd, MPI.INT, r, 0, rc, rd, MPI.INT)
    elif coll == "allgatherv":
        comm.Allgatherv(s, 0, sc[0], MPI.INT, r, 0, rc, rd, MPI.INT)
    elif coll == "gatherv":
        comm.Gatherv(s, 0, sc[0], MPI.INT, r, 0, rc, rd, MPI.INT, root)
    elif coll == "scatterv":
        comm.Scatterv(s, 0, sc, sd, MPI.INT, r, 0, rc[me], MPI.INT, root)
    elif coll == "allgather":
        comm.Allgather(s, 0, sc[0], MPI.INT, r, 0, rc[0], MPI.INT)
    else:
        comm.Alltoall(s, 0, sc[0], MPI.INT, r, 0, rc[0], MPI.INT)
