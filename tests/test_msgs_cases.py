"""CPU: the census of tests/msgs_cases.py against the planner of k_msgs and k_msgs_pool (no GPU).

tests/cpp/msgs_plan_test.cpp, built stand-alone under AddressSanitizer and UBSan, plans every case through plan_side
and plan_msg_seg (the functions the transport calls) and prints the segment it gives. The tests here assert that
each case plans to the cell it claims, that the union of cells is every one of the 32 bytes cells (16 shifts x 2
tiles) and the 40 granule cells (5 granules x source form x destination form x 2 tiles), that no layout leaves the
buffer the GPU test allocates, that no case is one k_transpose would take, and the lengths, counts and tile tails
the case table promises. Which tile a launch takes is launch_msgs' rule (csrc/mpjx_k_msgs.hip): the streaming
form from kStridedStreamBytes of batch payload, which the GPU test reaches with its ballast message.
"""
import os
import subprocess

import numpy as np
import pytest

import msgs_cases as MC
import pack_cases as PC
from test_strided_abi import build_and_run

SBUF, RBUF = 0x7F0000000000, 0x7F0000400000  # stand-ins for two 16-byte aligned allocations
COLS = ("kind", "glog", "stab", "dtab", "ngran", "bytes", "sh", "da", "tiles", "tiles_nt", "transpose", "slo", "shi",
        "dlo", "dhi")


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """[(case, {column: value})] for every case of the table."""
    tmp = tmp_path_factory.mktemp("msgs_plan")
    build_and_run(tmp, "msgs_plan_test", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    cases = MC.all_cases()
    text = "".join(c.describe() + "\n" for c in cases)
    r = subprocess.run([os.path.join(str(tmp), "msgs_plan_test"), "--cases"], input=text, capture_output=True,
                       text=True, timeout=600)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1] == f"msgs_plan_test: ok ({len(cases)} cases)", \
        (r.stdout[-2000:], r.stderr[-3000:])
    rows = [dict(zip(COLS, (int(x) for x in ln.split()))) for ln in lines[:-1]]
    assert len(rows) == len(cases) and all(len(row) == len(COLS) for row in rows)
    return list(zip(cases, rows))


def planned_cell(c, row):
    """The cell the planner's segment runs in, at the tile the case's batch is launched with."""
    if row["kind"] == 0:
        return ("bytes", row["sh"], c.tile)
    return ("granule", row["glog"], "irr" if row["stab"] else "reg", "irr" if row["dtab"] else "reg", c.tile)


def test_every_case_plans_to_its_cell(planned):
    assert len({c.id for c, _ in planned}) == len(planned), "two cases share an id"
    for c, row in planned:
        assert planned_cell(c, row) == c.cell, (c.id, row)
        assert row["bytes"] == c.nbytes == c.send.index().size, (c.id, row)
        assert (row["tiles"], row["tiles_nt"]) == (c.tiles("default"), c.tiles("nt")), (c.id, row)
        assert row["transpose"] == 0, (c.id, "k_transpose would take this message")
        assert (c.send.form, c.recv.form) == ("irr" if row["stab"] else "reg", "irr" if row["dtab"] else "reg") \
            or c.kind == "bytes", c.id
        if c.kind == "bytes":
            assert c.send.contiguous and c.recv.contiguous and c.nbytes == c.recv.size(), c.id
            assert c.shift(SBUF, RBUF) == (c.claim[1], row["da"]) == (row["sh"], (c.recv.off & 15)), (c.id, row)
        else:
            assert not (c.send.contiguous and c.recv.contiguous), c.id
            assert row["ngran"] << row["glog"] == c.nbytes, (c.id, row)
            assert c.granule(SBUF, RBUF) == c.claim[1], (c.id, "the restated granule rule disagrees with the claim")
            # the layouts alone cap the granule: the buffer positions are multiples of it
            assert PC.granule_log(c.send.layout_bytes() + c.recv.layout_bytes()) == c.claim[1], c.id
            assert c.send.off % (1 << c.claim[1]) == 0 and c.recv.off % (1 << c.claim[1]) == 0, c.id


def test_every_address_lies_inside_the_test_buffers(planned):
    for c, row in planned:
        for side, lo, hi in ((c.send, row["slo"], row["shi"]), (c.recv, row["dlo"], row["dhi"])):
            assert 0 <= lo < hi <= side.alloc() - MC.SLACK, (c.id, lo, hi, side.alloc())
            assert side.alloc() % 16 == 0
            idx = side.index()
            assert (idx.min(), idx.max() + 1) == (lo, hi), (c.id, "the case's own index spans otherwise")
        ridx = c.recv.index()
        assert np.unique(ridx).size == ridx.size, (c.id, "a self-overlapping layout cannot be received into")


def test_all_32_bytes_cells_and_all_40_granule_cells(planned):
    got = {planned_cell(c, row) for c, row in planned}
    bytes_cells = {("bytes", sh, tile) for sh in range(16) for tile in MC.TILES}
    granule_cells = {("granule", g, s, d, tile) for g in range(5) for s in MC.FORMS for d in MC.FORMS for tile in MC.TILES}
    assert len(bytes_cells) == 32 and len(granule_cells) == 40
    missing = sorted(map(str, (bytes_cells | granule_cells) - got))
    assert not missing, f"{len(missing)} cells are never run, the first: {missing[0]}"
    assert not got - bytes_cells - granule_cells, sorted(map(str, got - bytes_cells - granule_cells))
    # shift16's arms by name: q = sh >> 2 and b = sh & 3, each pair at both tiles
    assert {(sh >> 2, sh & 3, t) for _, sh, t in (x for x in got if x[0] == "bytes")} == \
        {(q, b, t) for q in range(4) for b in range(4) for t in MC.TILES}


def test_bytes_cells_have_the_lengths_that_can_break(planned):
    for tile in MC.TILES:
        t = 16 * MC.TILE[tile]
        for sh in range(16):
            mine = [(c, row) for c, row in planned if c.cell == ("bytes", sh, tile) and c.name.startswith("sh")]
            by_da = {}
            for c, row in mine:
                by_da.setdefault(row["da"], set()).add(c.nbytes)
            assert by_da.get(13, set()) >= {5}, (sh, tile)  # no whole vector, across a 16-byte line
            want = {16, t, t + 16, 2 * t - 1}
            assert by_da.get(0, set()) >= want, (sh, tile, "no head")
            other = [da for da in by_da if da and by_da[da] >= want]
            assert other, (sh, tile, "head and tail")
            for c, row in mine:
                if row["da"] == 0 and c.nbytes == t:  # one tile exactly
                    assert row["tiles_nt" if tile == "nt" else "tiles"] == 1, c.id
                if row["da"] == 0 and c.nbytes == t + 16:  # one tile and a vector
                    assert row["tiles_nt" if tile == "nt" else "tiles"] == 2, c.id


def test_sweep_has_all_256_alignment_pairs(planned):
    sweep = [(c, row) for c, row in planned if c.name.startswith("sweep")]
    assert len(sweep) == 256 == len({(c.send.off & 15, c.recv.off & 15) for c, _ in sweep})
    for c, row in sweep:
        assert c.tile == "default" and c.nbytes == MC.SWEEP_BYTES and row["tiles"] == 1
        head = (16 - row["da"]) & 15
        # 4099 = 256 x 16 + 3: whole vectors everywhere, a head but at alignment 0, a tail but at alignment 13
        assert (c.nbytes - head) // 16 >= 2 and (head > 0) == (row["da"] != 0), c.id
        assert ((c.nbytes - head) % 16 > 0) == (row["da"] != 13), c.id


def test_granule_cells_have_the_counts_around_the_tile(planned):
    for tile in MC.TILES:
        for g in range(5):
            for s in MC.FORMS:
                for d in MC.FORMS:
                    seen = {row["ngran"] for c, row in planned
                            if c.cell == ("granule", g, s, d, tile) and in_matrix(c)}
                    want = set(MC.granule_counts(tile)) - ({1} if s == "irr" else set())  # one granule is one run
                    assert seen >= want, (g, s, d, tile, sorted(want - seen))


def in_matrix(c):
    return c.name.startswith("g")


def test_irregular_sides_are_shuffled_and_of_the_claimed_granule(planned):
    for c, row in planned:
        if c.kind != "granule":
            continue
        G = 1 << c.claim[1]
        for side in (c.send, c.recv):
            if side.form != "irr":
                continue
            lens, disps = side.spec[1], side.spec[2]
            assert PC.granule_log(list(lens) + list(disps)) == c.claim[1], (c.id, "blocks of a wider granule")
            assert G in lens and len(lens) >= 3, c.id
            assert list(disps) != sorted(disps) and disps[0] != 0, (c.id, "packed in address order")
        if c.send.form == c.recv.form == "reg":  # k_transpose takes one granule per block and two items or more
            for side in (c.send, c.recv):
                assert side.contiguous or side.items == 1 or side.f.blocklen >= 2 * G, c.id


def test_short_cases_end_inside_the_last_receive_item_at_a_tile_edge(planned):
    short = [(c, row) for c, row in planned if c.short]
    assert sorted((c.claim[1], c.tile) for c, _ in short) == sorted((g, t) for g in range(5) for t in MC.TILES)
    for c, row in short:
        per_item = c.recv.f.size >> c.claim[1]
        assert row["ngran"] == MC.TILE[c.tile] and row["ngran"] % per_item != 0, c.id
        assert c.recv.items == -(-row["ngran"] // per_item) and c.recv.form == "irr", c.id


def test_streaming_cells_have_partial_last_tiles(planned):
    """Every case is sized for the tile it runs at; every streaming cell has cases whose last 512-lane tile is partial
    (the counts one below and one above the tile, and one granule or vector past two tiles) beside the one that
    fills its last tile exactly."""
    cells = {}
    for c, row in planned:
        if c.tile != "nt":
            continue
        n = row["ngran"] if c.kind == "granule" else (row["da"] + row["bytes"] + 15) >> 4
        assert n <= 2 * MC.TILE["nt"] + 1, (c.id, "larger than the 512-lane tile's edges need")
        cells.setdefault(c.cell, []).append(n % MC.TILE["nt"])
    assert len(cells) == 16 + 20
    for cell, tails in cells.items():
        assert sum(1 for t in tails if t) >= 3 and 0 in tails, (cell, tails)
        # one past the tile in both kinds; one short of it where the table's counts have it (the granule kind)
        assert ({1, MC.TILE["nt"] - 1} if cell[0] == "granule" else {1, 2}) <= set(tails), (cell, tails)


def test_full_table_and_batch_sizes():
    full = MC.full_table()
    assert len(full) == MC.MSGS_MAX + 1 and [c.kind for c in full] == ["bytes", "granule"] * 12 + ["bytes"]
    tiles = [min(c.tiles(), 2) for c in full]
    assert {(a, b) for a, b in zip(tiles, tiles[1:])} == {(1, 1), (1, 2), (2, 1), (2, 2)}
    assert {c.claim[1] for c in full if c.kind == "granule"} == set(range(5))
    assert {c.claim[2:] for c in full if c.kind == "granule"} == {(s, d) for s in MC.FORMS for d in MC.FORMS}
    for tile in MC.TILES:
        room = MC.MSGS_MAX - (tile == "nt")  # the ballast message takes one segment
        for sh in range(16):
            assert len(MC.bytes_cases(sh, tile)) <= room
        for g in range(5):
            assert len(MC.granule_cases(g, tile)) <= room
        pool = MC.pool_cases(tile)
        assert len(pool) <= room
        assert sorted(c.claim[1] for c in pool if c.kind == "bytes") == list(range(16))
        assert sorted(c.claim[1:] for c in pool if c.kind == "granule") == [(g, "irr", "irr") for g in range(5)]
    # the ballast alone reaches the threshold; no batch of cases comes near it without one
    assert sum(c.nbytes for c in MC.all_cases()) < MC.STREAM_BYTES
