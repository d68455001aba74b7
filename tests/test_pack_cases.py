"""CPU: the census of tests/pack_cases.py against the planner of k_pack (no GPU).

tests/cpp/pack_plan_test.cpp, built stand-alone under AddressSanitizer and UBSan, plans every case through
plan_pack_seg (the function mpjx_pack and mpjx_unpack call) and prints the cell it gives. The tests here assert
that each case lands in the cell it claims, that the union of cells is every one of the 224 that exist (14 arms x
4 address forms x pack / unpack x 2 tiles), that no case's layout leaves the buffer the GPU test allocates, and
the tile-tail and two-route conditions the case table promises. The launch rules restated below (which form a
table takes, from which payload the kernel streams) are launch_pack's, csrc/mpjx_k_pack.hip.
"""
import os
import subprocess

import numpy as np
import pytest

import pack_cases as PC
from test_strided_abi import build_and_run

STREAM_DEFAULT = 64 << 20  # kStridedStreamBytes
BUF, IMAGE = 0x7F0000000000, 0x7F0000400000  # stand-ins for two 16-byte aligned allocations


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """[(case, (glog, wlog, lin, tab, nb, ngran, lo, hi))] for the matrix's cases and the edge cases."""
    tmp = tmp_path_factory.mktemp("pack_plan")
    build_and_run(tmp, "pack_plan_test", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    cases = PC.all_cases() + PC.edge_cases()
    text = "".join(c.describe() + "\n" for c in cases)
    r = subprocess.run([os.path.join(str(tmp), "pack_plan_test"), "--cases"], input=text, capture_output=True,
                       text=True, timeout=600)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == f"pack_plan_test: ok ({len(cases)} cases)", \
        (r.stdout[-2000:], r.stderr[-3000:])
    rows = [tuple(int(x) for x in ln.split()) for ln in lines[:-1]]
    assert len(rows) == len(cases) and all(len(row) == 8 for row in rows)
    return list(zip(cases, rows))


def launched(c, row):
    """(glog, wlog, form, tile) as launch_pack chooses them from the planner's descriptor and the case's knobs."""
    glog, wlog, lin, tab, nb, ngran = row[:6]
    env = c.env()
    cap = min(max(int(env.get("MPJX_INDEXED_LDS_MAX_BLOCKS", PC.LDS_BLOCKS)), 0), PC.LDS_BLOCKS)
    stream = int(env["MPJX_STRIDED_NT_MIN_MIB"]) << 20 if "MPJX_STRIDED_NT_MIN_MIB" in env else STREAM_DEFAULT
    form = "lin" if lin else "reg" if not tab else "lds" if nb <= cap else "direct"
    return glog, wlog, form, "nt" if (ngran << glog) >= stream else "default"


def matrix(planned):
    n = len(PC.all_cases())
    return planned[:n]


def test_every_case_lands_in_its_cell(planned):
    assert len({c.id for c, _ in planned}) == len(planned), "two cases share an id"
    for c, row in planned:
        assert launched(c, row) == (*c.cell, c.tile), (c.id, row)
        assert row[5] == c.ngran, (c.id, row)
        assert c.glog(BUF, IMAGE) == c.arm[0], (c.id, "the restated granule rule disagrees with the claim")
        assert c.bsz == 1 << c.arm[1], c.id
        assert c.index().size << c.arm[1] == c.ngran << c.arm[0], c.id


def test_every_address_lies_inside_the_test_buffers(planned):
    for c, row in planned:
        lo, hi = row[6:]
        assert 0 <= lo < hi <= c.nelem() * c.bsz, (c.id, lo, hi, c.nelem() * c.bsz)
        idx = c.index()
        assert idx.min() * c.bsz == lo and (idx.max() + 1) * c.bsz == hi, (c.id, "the case's own index spans otherwise")
        assert np.unique(idx).size == idx.size, (c.id, "a self-overlapping layout cannot be unpacked into")


def test_all_224_cells_are_launched(planned):
    got = set()
    for c, row in matrix(planned):
        g, w, form, tile = launched(c, row)
        got |= {(g, w, form, direction, tile) for direction in ("pack", "unpack")}  # round_trip runs both
    want = {(g, w, form, direction, tile) for g, w in PC.ARMS for form in PC.FORMS for direction in ("pack", "unpack")
            for tile in PC.TILES}
    assert len(want) == 224
    missing = sorted(want - got)
    assert not missing, f"{len(missing)} cells are never launched, the first: {missing[0]}"
    assert not got - want, sorted(got - want)


def test_tile_tails(planned):
    cases = [c for c, _ in matrix(planned)]
    for form in PC.FORMS:
        seen = {c.ngran for c in cases if c.form == form and c.tile == "default"}
        assert set(PC.TILE_COUNTS) <= seen, (form, sorted(set(PC.TILE_COUNTS) - seen))
    for arm in PC.ARMS:
        mine = [c for c in cases if c.arm == arm]
        assert any(c.ngran % 256 for c in mine if c.tile == "default"), arm
        assert {c.form for c in mine if c.tile == "nt"} == set(PC.FORMS), arm
    assert {c.ngran % PC.NT_TILE for c in cases if c.tile == "nt"} == {1, 2, 3}
    for c in cases:
        if c.tile == "nt":
            assert c.ngran << c.arm[0] >= PC.NT_BYTES and c.ngran % PC.NT_TILE in (1, 2, 3), c.id
            # at most three 512-granule steps to the next count the layout's item divides
            assert c.ngran << c.arm[0] < PC.NT_BYTES + (4 * PC.NT_TILE << c.arm[0]), (c.id, "larger than the check needs")
        else:
            assert c.ngran in PC.TILE_COUNTS, c.id


def test_two_routes_to_every_arm_below_16_bytes(planned):
    cases = [c for c, _ in matrix(planned)]
    for c in cases:
        buf, pay = c.addresses(BUF, IMAGE)
        if c.route == "lengths":  # the layout alone caps the granule
            assert PC.granule_log(c.layout_bytes()) == c.arm[0] and PC.granule_log([buf, pay]) == 4, c.id
        elif c.route == "offset":  # only the buffer's element offset does
            assert PC.granule_log(c.layout_bytes() + [pay]) > c.arm[0] and PC.granule_log([buf]) == c.arm[0], c.id
        else:  # only the payload's address does
            assert PC.granule_log(c.layout_bytes() + [buf]) > c.arm[0] and PC.granule_log([pay]) == c.arm[0] == 3, c.id
    for arm in PC.ARMS:
        routes = {c.route for c in cases if c.arm == arm}
        assert routes == ({"lengths"} if arm[0] == 4 else {"lengths", "offset", "payload"} if arm[0] == 3
                          else {"lengths", "offset"}), (arm, routes)
    pairs = {(c.arm, c.form) for c in cases if c.base == "FLOAT2"}
    assert pairs == {(arm, form) for arm in ((3, 2), (4, 2)) for form in ("reg", "lds", "direct")}


def test_edge_cases_sit_on_the_lds_capacity(planned):
    edge = planned[len(PC.all_cases()):]
    assert sorted((c.nblocks(), c.form, c.tile) for c, _ in edge) == [
        (512, "lds", "default"), (512, "lds", "nt"), (513, "direct", "default"), (513, "direct", "nt")]
    for c, row in edge:
        assert row[3] == 1 and row[4] == c.nblocks() and not c.env().get("MPJX_INDEXED_LDS_MAX_BLOCKS"), c.id
        assert c.ngran > 2 * (PC.NT_TILE if c.tile == "nt" else 1024), c.id
