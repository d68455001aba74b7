"""Struct and resized types through each family of calls once, shared by tests/test_gpu_struct.py (multicore rank
threads on one device) and tests/struct_driver.py (the RCCL stand-in, where the exchange engines pack and unpack).

Every function runs on one rank of a world of P and returns a list of messages, empty when every WHOLE buffer, gaps
included, equals what numpy builds from the seeded inputs of all ranks (each rank can rebuild every rank's input).
"""
import numpy as np

from mpjexpress_amd.mpi import MPI, Datatype

SENT = -7.0


def column(R, ld, old=MPI.DOUBLE):
    """A column of a row-major matrix `ld` wide, resized to one element: `count` items are adjacent columns."""
    v = Datatype.Vector(R, 1, ld, old)
    t = Datatype.Struct([1, 1], [0, old.size], [v, MPI.UB])
    v.Free()
    return t


def matrix(rank, R, ld, salt=0):
    return np.random.default_rng(1000 * salt + rank).uniform(-1, 1, (R, ld))


def same(got, exp, what):
    return [] if np.array_equal(got.view(np.uint64), exp.view(np.uint64)) else [f"{what}: differs"]


def alltoall_transpose(torch, comm, P, R=19, k=5):
    """Rank i owns an R x (P k) matrix; Alltoall with the column send type and a contiguous receive type leaves
    rank j with, from every rank i, the transpose of i's panel j: the distributed transpose without a local pass."""
    me, ld = comm.Rank(), P * k + 2
    col = column(R, ld)
    try:
        s = torch.from_numpy(matrix(me, R, ld)).cuda().reshape(-1)
        r = torch.full((P * R * k + 2,), SENT, dtype=torch.float64, device="cuda")
        comm.Alltoall(s, 0, k, col, r, 1, R * k, MPI.DOUBLE)
        torch.cuda.synchronize()
        exp = np.full(P * R * k + 2, SENT)
        for i in range(P):
            exp[1 + i * R * k:1 + (i + 1) * R * k] = matrix(i, R, ld)[:, me * k:(me + 1) * k].T.ravel()
        bad = same(r.cpu().numpy(), exp, f"Alltoall transpose rank {me}/{P}")
        # and back: contiguous panels scattered into the columns of a sentinel matrix
        back = torch.full((R * ld,), SENT, dtype=torch.float64, device="cuda")
        comm.Alltoall(r, 1, R * k, MPI.DOUBLE, back, 0, k, col)
        torch.cuda.synchronize()
        exp2 = np.full((R, ld), SENT)
        exp2[:, :P * k] = matrix(me, R, ld)[:, :P * k]
        return bad + same(back.cpu().numpy(), exp2.ravel(), f"Alltoall transpose back rank {me}/{P}")
    finally:
        col.Free()


def scatter_gather_panels(torch, comm, P, R=11, k=3, root=0):
    """Scatterv hands rank j the columns j k .. j k + k of the root's matrix as a contiguous k x R block; Gatherv
    puts them back into a sentinel matrix at the root."""
    me, ld = comm.Rank(), P * k + 1
    col = column(R, ld)
    try:
        a = matrix(root, R, ld, salt=1)
        s = torch.from_numpy(a).cuda().reshape(-1)
        r = torch.full((R * k + 1,), SENT, dtype=torch.float64, device="cuda")
        comm.Scatterv(s, 0, [k] * P, [j * k for j in range(P)], col, r, 0, R * k, MPI.DOUBLE, root)
        torch.cuda.synchronize()
        exp = np.full(R * k + 1, SENT)
        exp[:R * k] = a[:, me * k:(me + 1) * k].T.ravel()
        bad = same(r.cpu().numpy(), exp, f"Scatterv panels rank {me}/{P}")
        back = torch.full((R * ld,), SENT, dtype=torch.float64, device="cuda")
        comm.Gatherv(r, 0, R * k, MPI.DOUBLE, back, 0, [k] * P, [j * k for j in range(P)], col, root)
        torch.cuda.synchronize()
        exp2 = np.full((R, ld), SENT)
        if me == root:
            exp2[:, :P * k] = a[:, :P * k]
        return bad + same(back.cpu().numpy(), exp2.ravel(), f"Gatherv panels rank {me}/{P}")
    finally:
        col.Free()


def gap_struct():
    """Elements 1, 2 and 5..7 of an item of 9 (UB at 9), LB at 0: an irregular Struct with a gap and padding."""
    return Datatype.Struct([2, 3, 1, 1], [1, 5, 0, 9], [MPI.DOUBLE, MPI.DOUBLE, MPI.LB, MPI.UB]), [1, 2, 5, 6, 7], 9


def bcast_struct(torch, comm, P, count=4, root=0):
    me = comm.Rank()
    t, idx, ext = gap_struct()
    try:
        assert (t.Size(), t.Extent(), t.Lb(), t.Ub()) == (5, 9, 0, 9)
        n = count * ext + 2
        src = np.random.default_rng(77).uniform(-1, 1, n)
        buf = torch.from_numpy(src if me == root else np.full(n, SENT)).cuda()
        comm.Bcast(buf, 1, count, t, root)
        torch.cuda.synchronize()
        exp = src.copy() if me == root else np.full(n, SENT)
        for k in range(count):
            for i in idx:
                exp[1 + k * ext + i] = src[1 + k * ext + i]
        return same(buf.cpu().numpy(), exp, f"Bcast of a Struct with a gap rank {me}/{P}")
    finally:
        t.Free()


def pack_round_trip(torch, comm, P, count=3):
    """Pack of a Struct gives the image of the Hindexed type with the same blocks; Unpack restores the blocks and
    nothing else."""
    me = comm.Rank()
    t, idx, ext = gap_struct()
    h = Datatype.Hindexed([2, 3], [1, 5], MPI.DOUBLE)  # the same blocks; its own extent is 7, so one item at a time
    try:
        n = count * ext + 1
        src = np.random.default_rng(5 + me).uniform(-1, 1, n)
        buf = torch.from_numpy(src).cuda()
        size = comm.Pack_size(count, t)
        img = torch.zeros(size + 8, dtype=torch.uint8, device="cuda")
        end = comm.Pack(buf, 0, count, t, img, 0)
        ref = torch.zeros(size + 8, dtype=torch.uint8, device="cuda")
        packed = torch.from_numpy(np.concatenate([src[k * ext + np.array(idx)] for k in range(count)])).cuda()
        rend = comm.Pack(packed, 0, count * 5, MPI.DOUBLE, ref, 0)
        bad = [] if (end == rend and torch.equal(img, ref)) else [f"Pack image rank {me}: differs from the packed elements'"]
        one = torch.zeros(comm.Pack_size(1, h) + 8, dtype=torch.uint8, device="cuda")
        one_s = torch.zeros_like(one)
        if not (comm.Pack(buf, 0, 1, h, one, 0) == comm.Pack(buf, 0, 1, t, one_s, 0) and torch.equal(one, one_s)):
            bad.append(f"Pack image rank {me}: one item differs from the Hindexed type's")
        out = torch.full((n,), SENT, dtype=torch.float64, device="cuda")
        if comm.Unpack(img, 0, out, 0, count, t) != end:
            bad.append("Unpack: position")
        exp = np.full(n, SENT)
        for k in range(count):
            exp[k * ext + np.array(idx)] = src[k * ext + np.array(idx)]
        return bad + same(out.cpu().numpy(), exp, f"Unpack into a Struct rank {me}/{P}")
    finally:
        t.Free()
        h.Free()


def allreduce_column(torch, comm, P, R=23, C=4):
    """Allreduce(SUM, DOUBLE) on C resized columns: bit for bit the contiguous call on the packed vectors."""
    me, ld = comm.Rank(), C + 2
    col = column(R, ld)
    try:
        a = matrix(me, R, ld, salt=2)
        s = torch.from_numpy(a).cuda().reshape(-1)
        r = torch.full((R * ld,), SENT, dtype=torch.float64, device="cuda")
        comm.Allreduce(s, 1, r, 1, C, col, MPI.SUM)
        ps = torch.from_numpy(np.ascontiguousarray(a[:, 1:1 + C].T).ravel()).cuda()
        pr = torch.zeros_like(ps)
        comm.Allreduce(ps, 0, pr, 0, R * C, MPI.DOUBLE, MPI.SUM)
        torch.cuda.synchronize()
        exp = np.full((R, ld), SENT)
        exp[:, 1:1 + C] = pr.cpu().numpy().reshape(C, R).T
        return same(r.cpu().numpy(), exp.ravel(), f"Allreduce on resized columns rank {me}/{P}")
    finally:
        col.Free()


FAMILIES = (alltoall_transpose, scatter_gather_panels, bcast_struct, pack_round_trip, allreduce_column)


def run_all(torch, comm, P):
    bad = []
    for fn in FAMILIES:
        bad += fn(torch, comm, P)
    return bad
