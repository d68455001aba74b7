"""GPU: the block-move collectives (Allgather(v), Gatherv, Scatterv, Alltoall(v)) in-process on device 0:
k_moves at P = 1 and in one-device multicore worlds (one launch by rank 0 for the whole world), and
SmpTransport's exchanges under MPJX_SMP_COPY=1. Every receive buffer starts as a sentinel and is compared
whole, byte for byte, against numpy indexing (tests/moves_cases.py); send buffers must come back unchanged."""
import os
import threading

import numpy as np
import pytest

import moves_cases as MC
from mpjexpress_amd import mpi
from mpjexpress_amd.mpi import MPI, MPIException

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LENGTHS = (0, 1, 15, 16, 17, 31, 33, 4099)
LONG = 70001  # several tiles
LONG_PAIRS = ((0, 0), (0, 1), (3, 3), (5, 12), (15, 8), (4, 8), (8, 4))


def run_ranks(comms, fn, limit=60):
    """fn(comm) on one thread per rank under a time limit; returns (results, errors) per rank."""
    P = len(comms)
    out, err = [None] * P, [None] * P

    def body(r):
        try:
            torch.cuda.set_device(0)
            out[r] = fn(comms[r])
        except BaseException as e:  # noqa: BLE001
            err[r] = e
    ts = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(P)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=limit)
    assert not any(t.is_alive() for t in ts), "a rank hung"
    return out, err


def world(P):
    return mpi.smp_world(P, [0] * P)


def free(comms):
    for c in comms:
        c.Free()


@pytest.fixture(scope="module")
def one():
    comms = world(1)
    yield comms[0]
    free(comms)


class Sweep:
    """One send and one receive allocation (16-B aligned) reused by every call of an alignment sweep."""

    def __init__(self, dt, nbytes):
        self.dt = dt
        self.td = MC.torch_dtype(torch, dt)
        self.host = np.random.default_rng(dt.code).integers(0, 256, nbytes, dtype=np.uint8)
        self.s = torch.from_numpy(self.host).cuda().view(self.td)
        self.r = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        assert self.s.data_ptr() % 16 == 0 and self.r.data_ptr() % 16 == 0
        self.calls = 0

    def move(self, comm, soff, a, roff, b, n):
        """P = 1 Alltoallv of n elements from displacement a to displacement b (Python offsets soff, roff in
        base elements); None, or what differs."""
        dt, esz, bs = self.dt, self.dt.byteSize, self.dt.baseSize
        lo, hi = roff * bs + b * esz, roff * bs + (b + n) * esz
        span = hi + 64
        self.r[:span].fill_(MC.SENT)
        comm.Alltoallv(self.s, soff, [n], [a], dt, self.r.view(self.td), roff, [n], [b], dt)
        self.calls += 1
        got = self.r[:span].cpu().numpy()
        exp = np.full(span, MC.SENT, np.uint8)
        src = soff * bs + a * esz
        exp[lo:hi] = self.host[src:src + n * esz]
        if np.array_equal(got, exp):
            return None
        bad = np.flatnonzero(got != exp)
        return f"{dt} a={a} b={b} soff={soff} roff={roff} n={n}: {bad.size} bytes differ, first at {bad[0]} (segment {lo}..{hi})"


def test_alignment_sweep_bytes(one):
    """Every (src mod 16, dst mod 16) pair at every length that takes another path through a tile: empty,
    inside one vector, head only, head + tail, whole vectors, and 70,001 bytes over several tiles."""
    sw = Sweep(MPI.BYTE, LONG + 256)
    bad = []
    for a in range(16):
        for b in range(16):
            for n in LENGTHS:
                bad.append(sw.move(one, 0, a, 0, b, n))
    for a, b in LONG_PAIRS:
        bad.append(sw.move(one, 0, a, 0, b, LONG))
    bad = [m for m in bad if m]
    assert not bad, bad[:10]
    assert sw.calls == 16 * 16 * len(LENGTHS) + len(LONG_PAIRS)
    assert np.array_equal(sw.s.view(torch.uint8).cpu().numpy(), sw.host), "the send buffer changed"


def test_alignment_sweep_int(one):
    sw = Sweep(MPI.INT, 4 * (LONG + 64))
    bad = [sw.move(one, 0, a, 0, b, n) for a in range(4) for b in range(4) for n in LENGTHS]
    bad += [sw.move(one, 0, a % 4, 0, b % 4, LONG) for a, b in LONG_PAIRS]
    bad = [m for m in bad if m]
    assert not bad, bad[:10]


def test_alignment_sweep_double2(one):
    """A DOUBLE2 element is 16 B: displacements keep the alignment, the Python offsets (8-B base elements) set it."""
    sw = Sweep(MPI.DOUBLE2, 16 * (4099 + 16))
    bad = [sw.move(one, so, a, ro, b, n) for so in (0, 1) for ro in (0, 1) for a in (0, 1) for b in (0, 1)
           for n in LENGTHS]
    bad = [m for m in bad if m]
    assert not bad, bad[:10]


def run_matrix(comms, tname, colls=MC.COLLS):
    P = len(comms)
    todo = [(coll, root, MC.make_case(coll, P, tname, root)) for coll, p_, t_, root in MC.matrix([P], [tname])
            if coll in colls]

    def body(c):
        return [MC.run_rank(torch, c, coll, ranks[c.Rank()], root) for coll, root, ranks in todo]
    out, err = run_ranks(comms, body)
    assert not any(err), err
    bad = [m for r in out for m in r if m]
    assert not bad, bad[:6]
    return len(todo)


@pytest.mark.parametrize("tname", list(MC.TYPES))
@pytest.mark.parametrize("P", [2, 3, 5, 8])
def test_six_collectives_ragged(P, tname):
    """count(i -> j) = 0 or 1 + (131 i + 71 j) % 97 elements, displacements with gaps and descending in
    rank order, offsets that are no multiple of 16 B; rooted calls at roots 0 and P - 1."""
    comms = world(P)
    try:
        assert run_matrix(comms, tname) == 8
    finally:
        free(comms)


def run_kat(comms):
    P = len(comms)
    cases = MC.kat_cases(P)

    def body(c):
        me, got = c.Rank(), []
        for name, coll, root, ranks, exp in cases:
            s = torch.from_numpy(ranks[me][0]).cuda()
            r = torch.zeros(ranks[me][5], dtype=torch.int32, device="cuda")
            MC.kat_call(c, coll, ranks[me], s, r, root)
            got.append(r.cpu().numpy())
        return got
    out, err = run_ranks(comms, body)
    assert not any(err), err
    for i, (name, coll, root, ranks, exp) in enumerate(cases):
        for me in range(P):
            assert np.array_equal(out[me][i], exp[me]), (name, me, out[me][i][:48], exp[me][:48])
    return cases, out


def test_reference_ccl_known_answers_at_3_tasks():
    """alltoallv.java, allgatherv.java and gatherv.java hold `ans` tables (tests/golden/ccl_moves_kat.json):
    the receive buffers must equal them; scatterv, allgather and alltoall hold rules, numpy evaluates them."""
    kat = MC.kat()
    comms = world(3)
    try:
        cases, out = run_kat(comms)
    finally:
        free(comms)
    idx = {name: i for i, (name, *_rest) in enumerate(cases)}
    for me in range(3):
        assert out[me][idx["alltoallv"]].tolist() == kat["alltoallv"]["ans"], me
        assert out[me][idx["allgatherv"]][:45].tolist() == kat["allgatherv"]["ans"], me
        assert not out[me][idx["allgatherv"]][45:].any()
    assert out[0][idx["gatherv"]][:45].tolist() == kat["gatherv"]["ans"]
    for me in (1, 2):
        assert not out[me][idx["gatherv"]].any(), "a non-root's receive buffer was written"


def test_more_segments_than_one_table():
    """Alltoall at P = 9 is 81 segments: two launches of rank 0 on one stream."""
    comms = world(9)
    try:
        ranks = MC.make_case("alltoall", 9, "INT", eq=1031)
        out, err = run_ranks(comms, lambda c: MC.run_rank(torch, c, "alltoall", ranks[c.Rank()]))
        assert not any(err), err
        assert not any(out), out
    finally:
        free(comms)


THRESH = 64 << 20  # k_moves' streaming form: 64 MiB per call, k_copies' threshold


@pytest.mark.parametrize("block", [THRESH // 2 - 4, THRESH // 2 + 4, THRESH // 8 - 4, THRESH // 8 + 4 * 3],
                         ids=["half-", "half+", "eighth-", "eighth+"])
def test_allgather_on_both_sides_of_the_streaming_threshold(block):
    """Allgather at P = 2, INT, receive offset one element. The world's one launch moves 4 blocks: blocks
    of an eighth of the threshold put it just under and just over 64 MiB; blocks of half of it (what one
    rank receives reaches the threshold) are both well inside the streaming form."""
    n = block // 4
    comms = world(2)
    g = torch.Generator("cuda").manual_seed(block)
    sends = [torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), dtype=torch.int32, device="cuda", generator=g) for _ in range(2)]
    keep = [s.clone() for s in sends]

    def body(c):
        r = torch.full((2 * n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        c.Allgather(sends[c.Rank()], 0, n, MPI.INT, r, 1, n, MPI.INT)
        return (bool(torch.equal(r[1:1 + n], keep[0])), bool(torch.equal(r[1 + n:1 + 2 * n], keep[1])),
                r[0].item() == 0x5A5A5A5A, bool((r[1 + 2 * n:] == 0x5A5A5A5A).all()))
    try:
        out, err = run_ranks(comms, body)
        assert not any(err), err
        assert out == [(True, True, True, True)] * 2, out
        assert all(torch.equal(a, b) for a, b in zip(sends, keep)), "a send buffer changed"
    finally:
        free(comms)


def test_smp_exchange_engine():
    """MPJX_SMP_COPY=1 (read per call): the same matrix at P = 3 through SmpTransport::exchange, the rank's
    own block by k_moves."""
    old = os.environ.get("MPJX_SMP_COPY")
    os.environ["MPJX_SMP_COPY"] = "1"
    comms = world(3)
    try:
        for tname in MC.TYPES:
            assert run_matrix(comms, tname) == 8
    finally:
        free(comms)
        if old is None:
            del os.environ["MPJX_SMP_COPY"]
        else:
            os.environ["MPJX_SMP_COPY"] = old


# ---- errors ---------------------------------------------------------------------------------------------
def _alltoallv(c, sc, rc, rd=None, n=64):
    P = c.Size()
    s = torch.zeros(n, dtype=torch.int32, device="cuda")
    r = torch.zeros(n, dtype=torch.int32, device="cuda")
    sd = [8 * j for j in range(P)]
    c.Alltoallv(s, 0, sc, sd, MPI.INT, r, 0, rc, rd or sd, MPI.INT)


def test_mismatched_counts_between_multicore_ranks_raise_on_every_rank():
    comms = world(2)
    try:
        # rank 0 sends 5 to rank 1, which expects 4
        out, err = run_ranks(comms, lambda c: _alltoallv(c, [3, 5], [4, 5] if c.Rank() == 1 else [3, 3]), limit=30)
        assert all(isinstance(e, MPIException) for e in err), err
        assert all("rank 0 sends 20 bytes to rank 1, which receives 16" in str(e) for e in err), err
    finally:
        free(comms)


def test_overlapping_receive_segments_fail_the_world():
    comms = world(3)
    try:
        def body(c):
            rd = [0, 2, 16] if c.Rank() == 1 else None  # rank 1: segments from ranks 0 and 1 overlap
            _alltoallv(c, [4, 4, 4], [4, 4, 4], rd)
        out, err = run_ranks(comms, body, limit=30)
        assert all(isinstance(e, MPIException) for e in err), err
        assert "overlap" in str(err[1]) and "(-1)" in str(err[1]), err[1]
    finally:
        free(comms)


def test_argument_errors(one):
    s = torch.zeros(64, dtype=torch.int32, device="cuda")
    r = torch.zeros(64, dtype=torch.int32, device="cuda")
    hs, hr = np.zeros(64, np.int32), np.zeros(64, np.int32)
    for call in (lambda: one.Allgather(hs, 0, 4, MPI.INT, hr, 0, 4, MPI.INT),
                 lambda: one.Alltoall(hs, 0, 4, MPI.INT, r, 0, 4, MPI.INT),
                 lambda: one.Alltoallv(s, 0, [4], [0], MPI.INT, hr, 0, [4], [0], MPI.INT),
                 lambda: one.Gatherv(hs, 0, 4, MPI.INT, hr, 0, [4], [0], MPI.INT, 0),
                 lambda: one.Scatterv(hs, 0, [4], [0], MPI.INT, hr, 0, 4, MPI.INT, 0),
                 lambda: one.Allgatherv(hs, 0, 4, MPI.INT, hr, 0, [4], [0], MPI.INT)):
        with pytest.raises(MPIException, match="device-resident"):
            call()
    with pytest.raises(MPIException, match="shorter"):
        one.Alltoallv(s, 0, [], [], MPI.INT, r, 0, [4], [0], MPI.INT)
    with pytest.raises(MPIException, match="differs"):
        one.Allgather(s, 0, 4, MPI.INT, r, 0, 4, MPI.FLOAT)


@pytest.mark.parametrize("case", ["negative_count", "negative_displacement", "in_place", "self_mismatch", "bad_root"])
def test_c_abi_rejections(case):
    """Each leaves a one-rank world failed, so each gets its own."""
    comms = world(1)
    c = comms[0]
    s = torch.zeros(64, dtype=torch.int32, device="cuda")
    r = torch.zeros(64, dtype=torch.int32, device="cuda")
    try:
        with pytest.raises(MPIException, match=r"\(-1\)"):
            if case == "negative_count":
                c.Alltoallv(s, 0, [-1], [0], MPI.INT, r, 0, [-1], [0], MPI.INT)
            elif case == "negative_displacement":
                c.Alltoallv(s, 0, [4], [-2], MPI.INT, r, 4, [4], [0], MPI.INT)
            elif case == "in_place":
                c.Alltoallv(s, 0, [8], [0], MPI.INT, s, 4, [8], [0], MPI.INT)
            elif case == "self_mismatch":
                c.Alltoallv(s, 0, [8], [0], MPI.INT, r, 0, [7], [0], MPI.INT)
            else:
                c.Gatherv(s, 0, 4, MPI.INT, r, 0, [4], [0], MPI.INT, 1)
    finally:
        free(comms)
