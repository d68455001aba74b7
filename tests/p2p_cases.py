"""Layouts and expected bytes of the point-to-point tests (tests/test_gpu_p2p.py, test_gpu_p2p_halo.py): a layout
is a datatype and the base-element indices one item packs, in pack order, computed here by numpy indexing."""
import json
import os

import numpy as np

from mpjexpress_amd.mpi import MPI, Datatype

SENT = 0xA5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pt2pt_kat.json")
TYPES = {"INT": MPI.INT, "FLOAT": MPI.FLOAT, "DOUBLE": MPI.DOUBLE}


def kat():
    return json.load(open(GOLDEN))


class Layout:
    """name, the library type, the indices of one item (base elements from its origin) and its extent"""

    def __init__(self, name, dt, idx, extent):
        self.name, self.dt, self.idx, self.extent = name, dt, np.asarray(idx, np.int64), extent
        assert dt.Size() == len(self.idx) and dt.Extent() == extent, (name, dt.Size(), len(self.idx), dt.Extent(), extent)

    def indices(self, items):
        """Base-element indices of `items` items in pack order."""
        return (np.arange(items, dtype=np.int64)[:, None] * self.extent + self.idx[None, :]).reshape(-1)

    def span(self, items):
        return int((items - 1) * self.extent + self.idx.max() + 1) if items > 0 and len(self.idx) else 0


def blocks(bl, ds):
    return np.concatenate([np.arange(d, d + b) for b, d in zip(bl, ds)]) if len(bl) else np.zeros(0, np.int64)


def layouts(base):
    """The six layout kinds of the matrix over `base`, with odd block lengths."""
    bl513 = [1 + i % 3 for i in range(513)]
    ds513 = [((i * 7) % 513) * 4 + 1 for i in range(513)]
    return [
        Layout("contiguous", base, [0], 1),
        Layout("vector", Datatype.Vector(5, 3, 7, base), blocks([3] * 5, [7 * j for j in range(5)]), 31),
        Layout("hvector", Datatype.Hvector(4, 2, 9, Datatype.Vector(2, 1, 2, base)),
               np.concatenate([np.array([0, 2, 3, 5]) + 9 * j for j in range(4)]), 33),
        Layout("indexed3", Datatype.Indexed([3, 1, 5], [7, 0, 20], base), blocks([3, 1, 5], [7, 0, 20]), 25),
        Layout("indexed513", Datatype.Indexed(bl513, ds513, base), blocks(bl513, ds513), max(d + b for b, d in zip(bl513, ds513)) - 1),
        Layout("struct_ub", Datatype.Struct([3, 1, 1], [0, 5, 9], [base, base, MPI.UB]), [0, 1, 2, 5], 9),
    ]


def torch_dtype(torch, dt):
    return getattr(torch, dt.torch_dtype_name)


def differs(got, exp, what):
    if np.array_equal(got, exp):
        return None
    bad = np.flatnonzero(got != exp)
    return f"{what}: {bad.size} bytes differ, first at {bad[0]}"
