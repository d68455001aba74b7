"""mpiJava-1.2 style host mirror of the reduction path, over libmpjx's C ABI.

Mirrors the reference's public surface for this path so that tests and callers read like the
reference's own programs (e.g. test/mpi/ccl/allreduce.java):

    MPI.SUM, MPI.DOUBLE, ...                     src/mpi/MPI.java:117-126, src/mpi/Datatype.java:57-66
    comm.Reduce(send, soff, recv, roff, count, datatype, op, root)      src/mpi/Intracomm.java:740-760
    comm.Allreduce(send, soff, recv, roff, count, datatype, op)          src/mpi/Intracomm.java:787-793
    comm.Reduce_scatter(send, soff, recv, roff, recvcounts, datatype, op) src/mpi/Intracomm.java:833-840
    comm.Scan(send, soff, recv, roff, count, datatype, op)               src/mpi/Intracomm.java:879-885
        (a derived datatype on device tensors: the mpjx_*_dt calls, element-wise over the packed sequence)
    comm.Bcast(buf, off, count, datatype, root), comm.Barrier(), comm.Rank(), comm.Size()
    comm.Allgather / Allgatherv / Gatherv / Scatterv / Alltoall / Alltoallv(sendbuf, sendoffset, sendcount[s],
        [sdispls,] sendtype, recvbuf, recvoffset, recvcount[s], [rdispls,] recvtype[, root])
                                                 src/mpi/Intracomm.java:363-690 (device tensors only)
    comm.Send / Recv / Isend / Irecv(buf, offset, count, datatype, dest | source, tag), comm.Sendrecv(sendbuf,
        sendoffset, sendcount, sendtype, dest, sendtag, recvbuf, recvoffset, recvcount, recvtype, source, recvtag),
        comm.Sendrecv_replace(buf, offset, count, datatype, dest, sendtag, source, recvtag); Request.Wait / Test /
        Is_null / Free / Waitall; Status.source / tag / Get_count / Get_elements;
        comm.Send_init / Recv_init(buf, offset, count, datatype, dest | source, tag) -> Prequest; Prequest.Start,
        Prequest.Startall(list) (src/mpi/Prequest.java)
                                                 src/mpi/Comm.java:381-2460, Request.java, Status.java (device tensors)
    comm.Pack_size(incount, datatype), comm.Pack(inbuf, offset, incount, datatype, outbuf, position),
    comm.Unpack(inbuf, position, outbuf, offset, outcount, datatype)     src/mpi/Comm.java:1860-1983
        (one mpjbuf section; the mpjbuf.Buffer is a torch.uint8 image on the device or in pinned memory)

Buffers are device-resident torch tensors (the device path) or numpy arrays (the host-resident
path, as Java heap arrays are). Offsets and counts are in elements. Calls block until the result is
in the receive buffer, like the Java methods. Errors raise MPIException (src/mpi/MPIException.java:42).
`MPI.isOldSelected` mirrors conf `mpjexpress.mpi.old.collectives` (src/mpi/MPI.java:70,266).
"""
import ctypes
import os
import struct
import threading

import numpy as np

from . import _lib

FLAG_OLD_COLLECTIVES = 0x1
FLAG_FAITHFUL = 0x2
FLAG_BLOCKING = 0x10  # the mpiJava calls are blocking: return complete (include/mpjx.h)


class MPIException(RuntimeError):
    pass


class Datatype:
    """A basic type, or a (value, index) pair type MPI.SHORT2..DOUBLE2 = Contiguous(2, base)
    (src/mpi/MPI.java:110-114). `code` is what crosses the C ABI (0x100 | base for pairs); offsets
    are in base elements (Java array indices), counts in datatype elements (pairs for *2 types)."""

    def __init__(self, base_type, name, np_dtype, torch_dtype_name, size=1):
        self.baseType = base_type
        self.name = name
        self.np_dtype = np.dtype(np_dtype)
        self.torch_dtype_name = torch_dtype_name
        self.size = size
        self.marker = size == 0  # MPI.LB / MPI.UB
        self.code = base_type if size <= 1 else (0x100 | base_type)
        self.baseSize = self.np_dtype.itemsize
        self.byteSize = self.baseSize * size
        self.extent = size  # base elements from one item to the next
        self.lb = 0  # the type's lb in base elements from an item's origin (0 for basic and regular types)
        self.ub = size  # and its ub: from the library for a derived type, never lb + extent computed here
        self.true_ub = size  # one past the highest base element an item touches (the ub unless bounds are explicit)
        self.derived = False

    @classmethod
    def _derived(cls, code, old, name):
        """The Datatype of a derived code the library handed out (mpjx_type_*)."""
        base, size, extent, lb = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        ub, tub = ctypes.c_int64(), ctypes.c_int64()
        _wrap("mpjx_type_info", code, ctypes.byref(base), ctypes.byref(size), ctypes.byref(extent))
        _wrap("mpjx_type_layout", code, ctypes.byref(lb), ctypes.byref(ub), None, None)
        _wrap("mpjx_type_true_bounds", code, None, ctypes.byref(tub))
        dt = cls(base.value, name, old.np_dtype, old.torch_dtype_name)
        dt.size, dt.extent, dt.lb, dt.code, dt.derived = size.value, extent.value, lb.value, code, True
        dt.ub, dt.true_ub = ub.value, tub.value
        dt.byteSize = dt.baseSize * dt.size
        return dt

    @classmethod
    def Contiguous(cls, count, oldtype):
        """Datatype.Contiguous (src/mpi/Contiguous.java): `count` items of oldtype in a row."""
        code = ctypes.c_int()
        _wrap("mpjx_type_contiguous", count, oldtype.code, ctypes.byref(code))
        return cls._derived(code.value, oldtype, f"Contiguous({count}, {oldtype.name})")

    @classmethod
    def Vector(cls, count, blocklength, stride, oldtype):
        """Datatype.Vector (src/mpi/Vector.java): `count` blocks of `blocklength` items of oldtype, `stride`
        items of oldtype apart. oldtype is basic, a pair type or contiguous; stride >= blocklength."""
        code = ctypes.c_int()
        _wrap("mpjx_type_vector", count, blocklength, stride, oldtype.code, ctypes.byref(code))
        return cls._derived(code.value, oldtype, f"Vector({count}, {blocklength}, {stride}, {oldtype.name})")

    @classmethod
    def Hvector(cls, count, blocklength, stride, oldtype):
        """Datatype.Hvector (src/mpi/Hvector.java): `count` blocks of `blocklength` items of oldtype, block j
        starting j * stride BASE elements from the origin. oldtype is any type."""
        code = ctypes.c_int()
        _wrap("mpjx_type_hvector", count, blocklength, stride, oldtype.code, ctypes.byref(code))
        return cls._derived(code.value, oldtype, f"Hvector({count}, {blocklength}, {stride}, {oldtype.name})")

    @classmethod
    def _indexed(cls, fn, name, blocklengths, displacements, oldtype):
        bl, ds = [int(x) for x in blocklengths], [int(x) for x in displacements]
        if len(bl) != len(ds):
            raise MPIException(f"{name}: {len(bl)} block lengths but {len(ds)} displacements")
        arr = ctypes.c_int64 * max(len(bl), 1)
        code = ctypes.c_int()
        _wrap(fn, len(bl), arr(*bl), arr(*ds), oldtype.code, ctypes.byref(code))
        return cls._derived(code.value, oldtype, f"{name}({bl}, {ds}, {oldtype.name})")

    @classmethod
    def Indexed(cls, array_of_blocklengths, array_of_displacements, oldtype):
        """Datatype.Indexed (src/mpi/Indexed.java): block i is blocklengths[i] items of oldtype starting
        displacements[i] extents of oldtype from the origin; packed in the arrays' order."""
        return cls._indexed("mpjx_type_indexed", "Indexed", array_of_blocklengths, array_of_displacements, oldtype)

    @classmethod
    def Hindexed(cls, array_of_blocklengths, array_of_displacements, oldtype):
        """Datatype.Hindexed (src/mpi/Hindexed.java): as Indexed, with displacements in BASE elements."""
        return cls._indexed("mpjx_type_hindexed", "Hindexed", array_of_blocklengths, array_of_displacements, oldtype)

    @classmethod
    def Struct(cls, array_of_blocklengths, array_of_displacements, array_of_types):
        """Datatype.Struct (src/mpi/Struct.java): block i is blocklengths[i] items of types[i] starting
        displacements[i] BASE elements from the origin; packed in the arrays' order. MPI.LB and MPI.UB set the
        bounds (the reference's order-dependent rules: include/mpjx.h); all other components share one base type."""
        bl, ds = [int(x) for x in array_of_blocklengths], [int(x) for x in array_of_displacements]
        ts = list(array_of_types)
        if not len(bl) == len(ds) == len(ts):
            raise MPIException(f"Struct: {len(bl)} block lengths, {len(ds)} displacements and {len(ts)} types")
        arr, codes = ctypes.c_int64 * max(len(bl), 1), ctypes.c_int * max(len(bl), 1)
        code = ctypes.c_int()
        _wrap("mpjx_type_struct", len(bl), arr(*bl), arr(*ds), codes(*[t.code for t in ts]), ctypes.byref(code))
        data = [t for t in ts if not t.marker]
        old = data[0] if data else MPI.BYTE
        return cls._derived(code.value, old, f"Struct({bl}, {ds}, {[t.name for t in ts]})")

    def Commit(self):
        pass

    def Free(self):
        """Release a derived type's code; the library rejects it in every later call."""
        if self.derived:
            _wrap("mpjx_type_free", self.code)

    def Size(self):
        return self.size

    def Extent(self):
        return self.extent

    def Lb(self):
        return self.lb

    def Ub(self):
        return self.ub

    def __repr__(self):
        return f"MPI.{self.name}"


class Op:
    def __init__(self, code, name):
        self.opCode = code
        self.name = name

    def __repr__(self):
        return f"MPI.{self.name}"


class MPI:
    BYTE = Datatype(1, "BYTE", np.int8, "int8")
    CHAR = Datatype(2, "CHAR", np.uint16, "uint16")
    SHORT = Datatype(3, "SHORT", np.int16, "int16")
    BOOLEAN = Datatype(4, "BOOLEAN", np.uint8, "uint8")
    INT = Datatype(5, "INT", np.int32, "int32")
    LONG = Datatype(6, "LONG", np.int64, "int64")
    FLOAT = Datatype(7, "FLOAT", np.float32, "float32")
    DOUBLE = Datatype(8, "DOUBLE", np.float64, "float64")
    SHORT2 = Datatype(3, "SHORT2", np.int16, "int16", 2)
    INT2 = Datatype(5, "INT2", np.int32, "int32", 2)
    LONG2 = Datatype(6, "LONG2", np.int64, "int64", 2)
    FLOAT2 = Datatype(7, "FLOAT2", np.float32, "float32", 2)
    DOUBLE2 = Datatype(8, "DOUBLE2", np.float64, "float64", 2)

    # an mpjbuf image, counted in bytes: the point-to-point calls only (include/mpjx.h "wire-format messages")
    PACKED = Datatype(9, "PACKED", np.uint8, "uint8")

    LB = Datatype(10, "LB", np.int8, "int8", 0)  # the bound markers: components of Datatype.Struct only
    UB = Datatype(11, "UB", np.int8, "int8", 0)

    MAX = Op(1, "MAX")
    MIN = Op(2, "MIN")
    SUM = Op(3, "SUM")
    PROD = Op(4, "PROD")
    LAND = Op(5, "LAND")
    BAND = Op(6, "BAND")
    LOR = Op(7, "LOR")
    BOR = Op(8, "BOR")
    LXOR = Op(9, "LXOR")
    BXOR = Op(10, "BXOR")
    MAXLOC = Op(11, "MAXLOC")
    MINLOC = Op(12, "MINLOC")

    ANY_SOURCE = -2  # src/mpi/MPI.java:132-136
    ANY_TAG = -2
    PROC_NULL = -3
    UNDEFINED = -1

    isOldSelected = False  # conf mpjexpress.mpi.old.collectives
    COMM_WORLD = None


DATATYPES = [MPI.BYTE, MPI.CHAR, MPI.SHORT, MPI.BOOLEAN, MPI.INT, MPI.LONG, MPI.FLOAT, MPI.DOUBLE]
OPS = [MPI.MAX, MPI.MIN, MPI.SUM, MPI.PROD, MPI.LAND, MPI.BAND, MPI.LOR, MPI.BOR, MPI.LXOR, MPI.BXOR,
       MPI.MAXLOC, MPI.MINLOC]
PAIR_TYPES = {0x103: MPI.SHORT2, 0x105: MPI.INT2, 0x106: MPI.LONG2, 0x107: MPI.FLOAT2, 0x108: MPI.DOUBLE2}


def datatype(code):
    """Datatype for a C-ABI type code (1..8, or 0x100 | base for the pair types)."""
    return PAIR_TYPES[code] if code in PAIR_TYPES else DATATYPES[code - 1]


def _wrap(fn, *args):
    try:
        _lib.call(fn, *args)
    except _lib.MPJXError as e:
        raise MPIException(str(e)) from None


def _is_torch(buf):
    t = getattr(_lib, "torch", None)
    return t is not None and isinstance(buf, t.Tensor)


def _dev_ptr(buf, off, dt, need):
    """Device address of base element `off` of a contiguous torch tensor of the datatype's base
    type, checking type and extent (`need` datatype elements)."""
    if not buf.is_cuda:
        raise MPIException("torch tensor buffers must be on a GPU device")
    if not buf.is_contiguous():
        raise MPIException("buffer must be contiguous")
    if buf.element_size() != dt.baseSize:
        raise MPIException(f"buffer element size {buf.element_size()} does not match {dt}")
    if off < 0 or off + need * dt.size > buf.numel():
        raise MPIException(f"offset {off} + count {need} exceeds buffer length {buf.numel()}")
    return buf.data_ptr() + off * dt.baseSize


def _dev_ptr_dt(buf, off, dt, count):
    """Device address of base element `off` for `count` items of the derived type dt: the buffer must hold
    the layout's true span ((count - 1) extents and one ub), not count * size elements."""
    span = (count - 1) * dt.extent + dt.true_ub if count > 0 and dt.size > 0 else 0
    if not buf.is_cuda:
        raise MPIException("torch tensor buffers must be on a GPU device")
    if not buf.is_contiguous():
        raise MPIException("buffer must be contiguous")
    if buf.element_size() != dt.baseSize:
        raise MPIException(f"buffer element size {buf.element_size()} does not match {dt}")
    if count < 0 or off < 0 or off + span > buf.numel():
        raise MPIException(f"offset {off} + layout span {span} of {count} x {dt} exceeds buffer length {buf.numel()}")
    return buf.data_ptr() + off * dt.baseSize


def _no_host_dt(name, dt):
    raise MPIException(f"{name}: the derived datatype {dt} is provided for device-resident buffers "
                       "(the *_host variants take basic and pair types)")


def _host_ptr(buf, off, dt, need):
    """Host address of base element `off` (numpy arrays of the base type, or of structured pairs)."""
    if not isinstance(buf, np.ndarray) or not buf.flags.c_contiguous:
        raise MPIException("host buffers must be C-contiguous numpy arrays")
    if buf.dtype.itemsize not in (dt.baseSize, dt.byteSize):
        raise MPIException(f"buffer dtype {buf.dtype} does not match {dt}")
    nbase = buf.size * (buf.dtype.itemsize // dt.baseSize)
    if off < 0 or off + need * dt.size > nbase:
        raise MPIException(f"offset {off} + count {need} exceeds buffer length {nbase}")
    return buf.ctypes.data + off * dt.baseSize


class Status:
    """mpi.Status (src/mpi/Status.java): source and tag of the matched message, and its length."""

    def __init__(self, st=None):
        self.source = st.source if st is not None else MPI.PROC_NULL
        self.tag = st.tag if st is not None else MPI.ANY_TAG
        self.error = st.error if st is not None else 0
        self._st = st if st is not None else _lib.Status(MPI.PROC_NULL, MPI.ANY_TAG, 0, 0, 0)

    def _counts(self, datatype):
        c, e = ctypes.c_int64(), ctypes.c_int64()
        _wrap("mpjx_get_count", ctypes.byref(self._st), datatype.code, ctypes.byref(c), ctypes.byref(e))
        return c.value, e.value

    def Get_count(self, datatype):
        """Received items of `datatype`, or MPI.UNDEFINED if the message is not a whole number of them."""
        return self._counts(datatype)[0]

    def Get_elements(self, datatype):
        """Received base elements."""
        return self._counts(datatype)[1]

    def wire_bytes(self):
        """Bytes of the image a Recv(MPI.PACKED) of the probed message needs (mpjx_wire_bytes)."""
        n = ctypes.c_int64()
        _wrap("mpjx_wire_bytes", ctypes.byref(self._st), ctypes.byref(n))
        return n.value


class Request:
    """mpi.Request (src/mpi/Request.java). The buffer belongs to the operation until Wait or a successful Test."""

    def __init__(self, comm, handle, buf):
        self._comm, self._h, self._buf = comm, ctypes.c_void_p(handle), buf

    def Is_null(self):
        return not self._h

    def Wait(self):
        st = _lib.Status()
        try:
            _wrap("mpjx_wait", ctypes.byref(self._h), ctypes.byref(st))
        finally:
            self._h, self._buf = ctypes.c_void_p(None), None
        return Status(st)

    def Test(self):
        """The Status if the operation is complete, else None. Never blocks."""
        st, flag = _lib.Status(), ctypes.c_int()
        _wrap("mpjx_test", ctypes.byref(self._h), ctypes.byref(flag), ctypes.byref(st))
        if not flag.value:
            return None
        self._buf = None
        return Status(st)

    def Free(self):
        _wrap("mpjx_request_free", ctypes.byref(self._h))
        self._buf = None

    @staticmethod
    def Waitall(array_of_requests):
        """Waits for every request (of one communicator); returns their Statuses in order."""
        reqs = list(array_of_requests)
        n = len(reqs)
        hs = (ctypes.c_void_p * max(n, 1))(*[r._h.value for r in reqs])
        sts = (_lib.Status * max(n, 1))()
        try:
            _wrap("mpjx_waitall", n, hs, sts)
        finally:
            for r in reqs:
                if not isinstance(r, Prequest):  # a persistent request stays, inactive
                    r._h, r._buf = ctypes.c_void_p(None), None
        return [Status(sts[i]) for i in range(n)]


class Prequest(Request):
    """mpi.Prequest (src/mpi/Prequest.java): a persistent request, made once by Comm.Send_init / Recv_init and
    activated by Start or Startall. Wait, Test and Waitall complete the activation and leave the request non-null
    and inactive; the buffer belongs to the request until Free."""

    def Start(self):
        if self._comm is not None:
            self._comm._sync_in(self._buf)  # what torch enqueued on the buffer precedes the message, as at Isend
        _wrap("mpjx_start", ctypes.byref(self._h))

    @staticmethod
    def Startall(array_of_requests):
        """Activates every request (of one communicator), in list order, in one call."""
        reqs = list(array_of_requests)
        n = len(reqs)
        hs = (ctypes.c_void_p * max(n, 1))(*[r._h.value for r in reqs])
        if reqs and reqs[0]._comm is not None:
            reqs[0]._comm._sync_in(*[r._buf for r in reqs])  # one synchronize for the whole list
        _wrap("mpjx_startall", n, hs)

    def Wait(self):
        st = _lib.Status()
        _wrap("mpjx_wait", ctypes.byref(self._h), ctypes.byref(st))
        return Status(st)

    def Test(self):
        st, flag = _lib.Status(), ctypes.c_int()
        _wrap("mpjx_test", ctypes.byref(self._h), ctypes.byref(flag), ctypes.byref(st))
        return Status(st) if flag.value else None

    def Is_active(self):
        p, a = ctypes.c_int(), ctypes.c_int()
        _wrap("mpjx_request_is_persistent", self._h, ctypes.byref(p), ctypes.byref(a))
        return bool(a.value)


class Intracomm:
    """One rank's view of a communicator (src/mpi/Intracomm.java)."""

    def __init__(self, handle, faithful=False):
        self._h = ctypes.c_void_p(handle)
        self.faithful = faithful
        r, s, d = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _wrap("mpjx_comm_rank", self._h, ctypes.byref(r))
        _wrap("mpjx_comm_size", self._h, ctypes.byref(s))
        _wrap("mpjx_comm_device", self._h, ctypes.byref(d))
        self._rank, self._size, self.device = r.value, s.value, d.value

    # -- mpiJava accessors
    def Rank(self):
        return self._rank

    def Size(self):
        return self._size

    @property
    def handle(self):
        return self._h

    def flags(self):
        f = FLAG_OLD_COLLECTIVES if MPI.isOldSelected else 0
        return f | (FLAG_FAITHFUL if self.faithful else 0) | FLAG_BLOCKING

    def Barrier(self):
        _wrap("mpjx_barrier", self._h)

    def Free(self):
        if self._h:
            _wrap("mpjx_comm_destroy", self._h)
            self._h = ctypes.c_void_p(None)

    def _sync_in(self, *bufs):
        if any(_is_torch(b) for b in bufs):
            _lib.torch.cuda.synchronize(self.device)

    def _sync_out(self):
        _wrap("mpjx_comm_synchronize", self._h)

    # -- communicator constructors: a new libmpjx world per sub-communicator, of the parent's engine
    # kind ("smp": rank threads of this process; "rccl": one process per GPU over RCCL; "ipc": processes
    # mapping each other's buffers). NativeIntracomm.java:160-215 keeps Split/Create on its strategy.
    _kind = "smp"

    def _world_base(self):
        """128 random bytes drawn by rank 0 and broadcast (device Bcast) to every rank."""
        torch = _lib.torch
        dev = torch.device("cuda", self.device)
        base = torch.zeros(128, dtype=torch.int8, device=dev)
        if self._rank == 0:
            base.copy_(torch.frombuffer(bytearray(os.urandom(128)), dtype=torch.int8))
        self.Bcast(base, 0, 128, MPI.BYTE, 0)
        return bytes(base.cpu().numpy().view(np.uint8))

    def _world_id(self, members):
        """Collective: the 128-byte id of this rank's new world (None outside every new group). Multicore
        worlds derive theirs from one shared random base (made unique per group by _sub_world); the
        process engines take their group leader's: an RCCL unique id (mpjx_get_unique_id, whose
        bootstrap root lives in the leader's process) or random bytes (IPC), gathered to every rank."""
        if self._kind == "smp":
            return self._world_base()
        leader = members[0] if members else None
        mine = bytes(128)
        if self._rank == leader:
            mine = unique_id() if self._kind == "rccl" else os.urandom(128)
        table = self._all_bytes(mine)
        return table[leader] if members else None

    def _sub_world(self, members, tag, base):
        """The world of `members` (parent ranks, in new-rank order) on their devices."""
        if self._rank not in members:
            return None
        h = ctypes.c_void_p()
        me = members.index(self._rank)
        if self._kind == "rccl":
            _wrap("mpjx_comm_init_rank", ctypes.byref(h), len(members), base, me, self.device)
        elif self._kind == "ipc":
            _wrap("mpjx_comm_init_ipc", ctypes.byref(h), len(members), base, me, self.device)
        else:
            uid = bytearray(base)
            for i, b in enumerate(struct.pack("<q", tag)):
                uid[i] ^= b
            devs = (ctypes.c_int * len(members))(*[self._devices[m] for m in members])
            _wrap("mpjx_comm_init_smp_rank", ctypes.byref(h), len(members), bytes(uid), me, devs)
        c = Intracomm(h.value, faithful=self.faithful)
        c._kind = self._kind
        c._devices = [self._devices[m] for m in members]
        return c

    def _all_ints(self, vals):
        """Every rank's int32 row (gathered to rank 0 on the device, then broadcast)."""
        torch = _lib.torch
        dev = torch.device("cuda", self.device)
        k, P = len(vals), self._size
        mine = torch.tensor(vals, dtype=torch.int32, device=dev)
        table = torch.zeros(k * P, dtype=torch.int32, device=dev)
        Gather(self, mine, 0, k, table, 0, k, MPI.INT, 0)
        self.Bcast(table, 0, k * P, MPI.INT, 0)
        return table.cpu().numpy().reshape(P, k)

    def _all_bytes(self, b):
        """Every rank's byte string of len(b) (all equal), gathered and broadcast on the device."""
        torch = _lib.torch
        dev = torch.device("cuda", self.device)
        k, P = len(b), self._size
        mine = torch.frombuffer(bytearray(b), dtype=torch.int8).to(dev)
        table = torch.zeros(k * P, dtype=torch.int8, device=dev)
        Gather(self, mine, 0, k, table, 0, k, MPI.BYTE, 0)
        self.Bcast(table, 0, k * P, MPI.BYTE, 0)
        t = table.cpu().numpy().view(np.uint8).reshape(P, k)
        return [bytes(t[r]) for r in range(P)]

    def Split(self, color, key):
        """Intracomm.Split (src/mpi/PureIntracomm.java:201-280; NativeIntracomm.java:160-170 keeps the
        result on its strategy, as this does): ranks of one color form a communicator ordered by key,
        ties by parent rank; a negative color (MPI.UNDEFINED) gets None. Collective."""
        t = self._all_ints([color, key, self.device])
        self._devices = [int(d) for d in t[:, 2]]
        members = None
        if color >= 0:
            members = sorted((r for r in range(self._size) if t[r, 0] == color), key=lambda r: (t[r, 1], r))
        base = self._world_id(members)
        if color < 0:
            return None
        return self._sub_world(members, int(color), base)

    def Create(self, group):
        """Intracomm.Create (src/mpi/PureIntracomm.java:302-309; NativeIntracomm.java:200-215): `group`
        lists the parent ranks of the new communicator in new-rank order (mpi.Group's members, the same
        on every rank); ranks outside it get None. Collective."""
        members = [int(m) for m in group]
        t = self._all_ints([self.device])
        self._devices = [int(d) for d in t[:, 0]]
        base = self._world_id(members if self._rank in members else None)
        return self._sub_world(members, -1, base)

    # -- reductions
    def Reduce(self, sendbuf, sendoffset, recvbuf, recvoffset, count, datatype, op, root):
        """recvbuf is significant at the root; with faithful=True every rank's recvbuf is left as
        PureIntracomm leaves it (MST: the rank's sub-tree partial, FT: its own send copy)."""
        is_root = self._rank == root
        if datatype.derived:
            if not _is_torch(sendbuf):
                _no_host_dt("Reduce", datatype)
            self._sync_in(sendbuf)
            sp = _dev_ptr_dt(sendbuf, sendoffset, datatype, count)
            rp = _dev_ptr_dt(recvbuf, recvoffset, datatype, count) if is_root else None
            _wrap("mpjx_reduce_dt", self._h, sp, rp, count, datatype.code, op.opCode, root, self.flags(), None)
            self._sync_out()
        elif _is_torch(sendbuf):
            self._sync_in(sendbuf)
            sp = _dev_ptr(sendbuf, sendoffset, datatype, count)
            rp = _dev_ptr(recvbuf, recvoffset, datatype, count) if (is_root or self.faithful) else None
            _wrap("mpjx_reduce", self._h, sp, rp, count, datatype.code, op.opCode, root,
                  self.flags(), None)
            self._sync_out()
        else:
            sp = _host_ptr(sendbuf, sendoffset, datatype, count)
            rp = _host_ptr(recvbuf, recvoffset, datatype, count) if (is_root or self.faithful) else None
            _wrap("mpjx_reduce_host", self._h, sp, rp, count, datatype.code, op.opCode, root,
                  self.flags())

    def Allreduce(self, sendbuf, sendoffset, recvbuf, recvoffset, count, datatype, op):
        if datatype.derived:
            if not _is_torch(sendbuf):
                _no_host_dt("Allreduce", datatype)
            self._sync_in(sendbuf, recvbuf)
            sp = _dev_ptr_dt(sendbuf, sendoffset, datatype, count)
            rp = _dev_ptr_dt(recvbuf, recvoffset, datatype, count)
            _wrap("mpjx_allreduce_dt", self._h, sp, rp, count, datatype.code, op.opCode, self.flags(), None)
            self._sync_out()
        elif _is_torch(sendbuf):
            self._sync_in(sendbuf, recvbuf)
            sp = _dev_ptr(sendbuf, sendoffset, datatype, count)
            rp = _dev_ptr(recvbuf, recvoffset, datatype, count)
            _wrap("mpjx_allreduce", self._h, sp, rp, count, datatype.code, op.opCode,
                  self.flags(), None)
            self._sync_out()
        else:
            sp = _host_ptr(sendbuf, sendoffset, datatype, count)
            rp = _host_ptr(recvbuf, recvoffset, datatype, count)
            _wrap("mpjx_allreduce_host", self._h, sp, rp, count, datatype.code, op.opCode,
                  self.flags())

    def Reduce_scatter(self, sendbuf, sendoffset, recvbuf, recvoffset, recvcounts, datatype, op):
        counts = list(recvcounts)[: self._size]
        if len(counts) < self._size:
            raise MPIException("recvcounts shorter than the communicator")
        rc = (ctypes.c_int64 * self._size)(*counts)
        total, mine = sum(counts), counts[self._rank]  # datatype elements
        if datatype.derived:
            if not _is_torch(sendbuf):
                _no_host_dt("Reduce_scatter", datatype)
            self._sync_in(sendbuf, recvbuf)
            sp = _dev_ptr_dt(sendbuf, sendoffset, datatype, total)
            rp = _dev_ptr_dt(recvbuf, recvoffset, datatype, mine)
            _wrap("mpjx_reduce_scatter_dt", self._h, sp, rp, rc, datatype.code, op.opCode, self.flags(), None)
            self._sync_out()
        elif _is_torch(sendbuf):
            self._sync_in(sendbuf, recvbuf)
            sp = _dev_ptr(sendbuf, sendoffset, datatype, total)
            rp = _dev_ptr(recvbuf, recvoffset, datatype, mine)
            _wrap("mpjx_reduce_scatter", self._h, sp, rp, rc, datatype.code, op.opCode,
                  self.flags(), None)
            self._sync_out()
        else:
            sp = _host_ptr(sendbuf, sendoffset, datatype, total)
            rp = _host_ptr(recvbuf, recvoffset, datatype, mine)
            _wrap("mpjx_reduce_scatter_host", self._h, sp, rp, rc, datatype.code, op.opCode,
                  self.flags())

    def Scan(self, sendbuf, sendoffset, recvbuf, recvoffset, count, datatype, op):
        if datatype.derived:
            if not _is_torch(sendbuf):
                _no_host_dt("Scan", datatype)
            self._sync_in(sendbuf, recvbuf)
            sp = _dev_ptr_dt(sendbuf, sendoffset, datatype, count)
            rp = _dev_ptr_dt(recvbuf, recvoffset, datatype, count)
            _wrap("mpjx_scan_dt", self._h, sp, rp, count, datatype.code, op.opCode, self.flags(), None)
            self._sync_out()
        elif _is_torch(sendbuf):
            self._sync_in(sendbuf, recvbuf)
            sp = _dev_ptr(sendbuf, sendoffset, datatype, count)
            rp = _dev_ptr(recvbuf, recvoffset, datatype, count)
            _wrap("mpjx_scan", self._h, sp, rp, count, datatype.code, op.opCode, self.flags(),
                  None)
            self._sync_out()
        else:
            sp = _host_ptr(sendbuf, sendoffset, datatype, count)
            rp = _host_ptr(recvbuf, recvoffset, datatype, count)
            _wrap("mpjx_scan_host", self._h, sp, rp, count, datatype.code, op.opCode,
                  self.flags())

    def Gather(self, sendbuf, sendoffset, sendcount, recvbuf, recvoffset, recvcount, datatype, root):
        Gather(self, sendbuf, sendoffset, sendcount, recvbuf, recvoffset, recvcount, datatype, root)

    def Scatter(self, sendbuf, sendoffset, sendcount, recvbuf, recvoffset, recvcount, datatype, root):
        Scatter(self, sendbuf, sendoffset, sendcount, recvbuf, recvoffset, recvcount, datatype, root)

    # -- block moves (src/mpi/Intracomm.java:363-690): device tensors; counts, displacements and offsets
    # in elements. One k_moves launch at P = 1 and in one-device multicore worlds, the transport's
    # exchanges elsewhere (include/mpjx.h).
    def _moves(self, name, sendbuf, sendtype, recvbuf, recvtype):
        """True if the call takes the strided path (mpjx_alltoallv_dt): a derived type on either side, or two
        different types of one base type. Two equal basic or pair types take the path they always took."""
        if sendtype.baseType != recvtype.baseType:
            raise MPIException(f"{name}: sendtype {sendtype} differs from recvtype {recvtype} in its base type")
        for b in (sendbuf, recvbuf):
            if b is not None and not _is_torch(b):
                raise MPIException(f"{name} is provided for device-resident buffers")
        self._sync_in(*(b for b in (sendbuf, recvbuf) if b is not None))
        return sendtype.derived or recvtype.derived or sendtype.code != recvtype.code

    def _dt_side(self, name, buf, off, dt, counts, displs):
        """(address, counts, displacements) of one side of mpjx_alltoallv_dt: counts in items of dt,
        displacements in base elements; the buffer must hold every layout's true span."""
        P = self._size
        c, d = [int(x) for x in counts][:P], [int(x) for x in displs][:P]
        if len(c) < P or len(d) < P:
            raise MPIException(f"{name}: counts or displacements shorter than the communicator")
        arr = ctypes.c_int64 * P
        span = max([dj + (cj - 1) * dt.extent + dt.true_ub for cj, dj in zip(c, d) if cj > 0 and dt.size > 0] or [0])
        if span == 0 and buf is None:
            return None, arr(*c), arr(*d)
        if not buf.is_cuda:
            raise MPIException("torch tensor buffers must be on a GPU device")
        if not buf.is_contiguous():
            raise MPIException("buffer must be contiguous")
        if buf.element_size() != dt.baseSize:
            raise MPIException(f"buffer element size {buf.element_size()} does not match {dt}")
        if off < 0 or min(d) < 0 or off + span > buf.numel():
            raise MPIException(f"{name}: offset {off} + layout span {span} exceeds buffer length {buf.numel()}")
        return buf.data_ptr() + off * dt.baseSize, arr(*c), arr(*d)

    def _dt(self, name, sendbuf, soff, sc, sd, stype, recvbuf, roff, rc, rd, rtype):
        sp, sca, sda = self._dt_side(name, sendbuf, soff, stype, sc, sd)
        rp, rca, rda = self._dt_side(name, recvbuf, roff, rtype, rc, rd)
        _wrap("mpjx_alltoallv_dt", self._h, sp, sca, sda, stype.code, rp, rca, rda, rtype.code, None)
        self._sync_out()

    def _equal(self, name, sendcount, sendtype, recvcount, recvtype):
        if sendcount * sendtype.size != recvcount * recvtype.size:
            raise MPIException(f"{name}: {sendcount} x {sendtype} and {recvcount} x {recvtype} differ in length")

    def _table(self, name, counts, displs):
        """(counts, displs as int64 arrays, elements spanned) of one rank's count/displacement lists."""
        c, d = [int(x) for x in counts][: self._size], [int(x) for x in displs][: self._size]
        if len(c) < self._size or len(d) < self._size:
            raise MPIException(f"{name}: counts or displacements shorter than the communicator")
        span = max([dj + cj for cj, dj in zip(c, d) if cj > 0] or [0])
        arr = ctypes.c_int64 * self._size
        return arr(*c), arr(*d), span

    def Allgather(self, sendbuf, sendoffset, sendcount, sendtype, recvbuf, recvoffset, recvcount, recvtype):
        if self._moves("Allgather", sendbuf, sendtype, recvbuf, recvtype):
            self._equal("Allgather", sendcount, sendtype, recvcount, recvtype)
            P, z = self._size, [0] * self._size
            return self._dt("Allgather", sendbuf, sendoffset, [sendcount] * P, z, sendtype, recvbuf, recvoffset,
                            [recvcount] * P, [j * recvcount * recvtype.extent for j in range(P)], recvtype)
        if sendcount != recvcount:
            raise MPIException("Allgather: sendcount must equal recvcount")
        sp = _dev_ptr(sendbuf, sendoffset, sendtype, sendcount)
        rp = _dev_ptr(recvbuf, recvoffset, recvtype, recvcount * self._size)
        _wrap("mpjx_allgather", self._h, sp, rp, sendcount, sendtype.code, None)
        self._sync_out()

    def Allgatherv(self, sendbuf, sendoffset, sendcount, sendtype, recvbuf, recvoffset, recvcount, displs,
                   recvtype):
        if self._moves("Allgatherv", sendbuf, sendtype, recvbuf, recvtype):
            P = self._size
            return self._dt("Allgatherv", sendbuf, sendoffset, [sendcount] * P, [0] * P, sendtype, recvbuf,
                            recvoffset, recvcount, displs, recvtype)
        rc, rd, span = self._table("Allgatherv", recvcount, displs)
        sp = _dev_ptr(sendbuf, sendoffset, sendtype, sendcount)
        rp = _dev_ptr(recvbuf, recvoffset, recvtype, span)
        _wrap("mpjx_allgatherv", self._h, sp, sendcount, rp, rc, rd, sendtype.code, None)
        self._sync_out()

    def Gatherv(self, sendbuf, sendoffset, sendcount, sendtype, recvbuf, recvoffset, recvcount, displs,
                recvtype, root):
        """recvbuf, recvcount and displs are significant at the root only."""
        is_root = self._rank == root
        if self._moves("Gatherv", sendbuf, sendtype, recvbuf if is_root else None, recvtype):
            z = [0] * self._size
            return self._dt("Gatherv", sendbuf, sendoffset, [sendcount if j == root else 0 for j in range(self._size)],
                            z, sendtype, recvbuf if is_root else None, recvoffset, recvcount if is_root else z,
                            displs if is_root else z, recvtype)
        rc = rd = rp = None
        if is_root:
            rc, rd, span = self._table("Gatherv", recvcount, displs)
            rp = _dev_ptr(recvbuf, recvoffset, recvtype, span)
        sp = _dev_ptr(sendbuf, sendoffset, sendtype, sendcount)
        _wrap("mpjx_gatherv", self._h, sp, sendcount, rp, rc, rd, sendtype.code, root, None)
        self._sync_out()

    def Scatterv(self, sendbuf, sendoffset, sendcount, displs, sendtype, recvbuf, recvoffset, recvcount,
                 recvtype, root):
        """sendbuf, sendcount and displs are significant at the root only."""
        is_root = self._rank == root
        if self._moves("Scatterv", sendbuf if is_root else None, sendtype, recvbuf, recvtype):
            z = [0] * self._size
            return self._dt("Scatterv", sendbuf if is_root else None, sendoffset, sendcount if is_root else z,
                            displs if is_root else z, sendtype, recvbuf, recvoffset,
                            [recvcount if j == root else 0 for j in range(self._size)], z, recvtype)
        sc = sd = sp = None
        if is_root:
            sc, sd, span = self._table("Scatterv", sendcount, displs)
            sp = _dev_ptr(sendbuf, sendoffset, sendtype, span)
        rp = _dev_ptr(recvbuf, recvoffset, recvtype, recvcount)
        _wrap("mpjx_scatterv", self._h, sp, sc, sd, rp, recvcount, sendtype.code, root, None)
        self._sync_out()

    def Alltoall(self, sendbuf, sendoffset, sendcount, sendtype, recvbuf, recvoffset, recvcount, recvtype):
        if self._moves("Alltoall", sendbuf, sendtype, recvbuf, recvtype):
            self._equal("Alltoall", sendcount, sendtype, recvcount, recvtype)
            P = self._size
            return self._dt("Alltoall", sendbuf, sendoffset, [sendcount] * P,
                            [j * sendcount * sendtype.extent for j in range(P)], sendtype, recvbuf, recvoffset,
                            [recvcount] * P, [j * recvcount * recvtype.extent for j in range(P)], recvtype)
        if sendcount != recvcount:
            raise MPIException("Alltoall: sendcount must equal recvcount")
        sp = _dev_ptr(sendbuf, sendoffset, sendtype, sendcount * self._size)
        rp = _dev_ptr(recvbuf, recvoffset, recvtype, recvcount * self._size)
        _wrap("mpjx_alltoall", self._h, sp, rp, sendcount, sendtype.code, None)
        self._sync_out()

    def Alltoallv(self, sendbuf, sendoffset, sendcount, sdispls, sendtype, recvbuf, recvoffset, recvcount,
                  rdispls, recvtype):
        if self._moves("Alltoallv", sendbuf, sendtype, recvbuf, recvtype):
            return self._dt("Alltoallv", sendbuf, sendoffset, sendcount, sdispls, sendtype, recvbuf, recvoffset,
                            recvcount, rdispls, recvtype)
        sc, sd, sspan = self._table("Alltoallv", sendcount, sdispls)
        rc, rd, rspan = self._table("Alltoallv", recvcount, rdispls)
        sp = _dev_ptr(sendbuf, sendoffset, sendtype, sspan)
        rp = _dev_ptr(recvbuf, recvoffset, recvtype, rspan)
        _wrap("mpjx_alltoallv", self._h, sp, sc, sd, rp, rc, rd, sendtype.code, None)
        self._sync_out()

    MOVE_KERNEL_MOVES, MOVE_KERNEL_STRIDED, MOVE_KERNEL_INDEXED, MOVE_KERNEL_TRANSPOSE = 1, 2, 4, 8

    def last_move_kernels(self):
        """The kernels this rank's last data-movement call launched (mpjx_comm_last_move_kernels): an OR of
        MOVE_KERNEL_*; 0 on a rank that launched nothing (rank 0 launches for a multicore world on one device)."""
        m = ctypes.c_uint()
        _wrap("mpjx_comm_last_move_kernels", self._h, ctypes.byref(m))
        return m.value

    # -- Pack / Unpack / Pack_size (src/mpi/Comm.java:1860-1983): one mpjbuf section from, or into, items of any
    # datatype on a device tensor. The image (mpjbuf.Buffer there) is a torch.uint8 tensor on the device or in
    # pinned host memory; positions are bytes. Local calls (include/mpjx.h).
    def Pack_size(self, incount, datatype):
        n = ctypes.c_int64()
        _wrap("mpjx_pack_size", incount, datatype.code, ctypes.byref(n))
        return n.value

    def _image(self, name, img):
        torch = _lib.torch
        if not _is_torch(img) or img.dtype != torch.uint8 or not img.is_contiguous():
            raise MPIException(f"{name}: the image must be a contiguous torch.uint8 tensor")
        if not (img.is_cuda or img.is_pinned()):
            raise MPIException(f"{name}: the image must be on the device or in pinned host memory")
        return img.data_ptr(), img.numel()

    def Pack(self, inbuf, offset, incount, datatype, outbuf, position):
        """Packs incount items of datatype from inbuf (base element `offset` on) into the image outbuf as one
        section at round_up(position, 8); returns the new position."""
        if not _is_torch(inbuf):
            raise MPIException("Pack is provided for device-resident buffers")
        ip, nb = self._image("Pack", outbuf)
        self._sync_in(inbuf, outbuf)
        p = _dev_ptr_dt(inbuf, offset, datatype, incount)
        pos = ctypes.c_int64(position)
        _wrap("mpjx_pack", self._h, p, incount, datatype.code, ip, nb, ctypes.byref(pos), None)
        self._sync_out()
        return pos.value

    def Unpack(self, inbuf, position, outbuf, offset, outcount, datatype):
        """Unpacks the section at round_up(position, 8) of the image inbuf into outcount items of datatype in
        outbuf (base element `offset` on); returns the new position. A section of another type or count, or one
        that passes the end of the image, raises MPIException and leaves outbuf untouched."""
        if not _is_torch(outbuf):
            raise MPIException("Unpack is provided for device-resident buffers")
        ip, nb = self._image("Unpack", inbuf)
        self._sync_in(inbuf, outbuf)
        p = _dev_ptr_dt(outbuf, offset, datatype, outcount)
        torch = _lib.torch
        status = torch.zeros(1, dtype=torch.int32, device=torch.device("cuda", self.device))
        torch.cuda.synchronize(self.device)
        pos = ctypes.c_int64(position)
        _wrap("mpjx_unpack", self._h, ip, nb, ctypes.byref(pos), p, outcount, datatype.code, status.data_ptr(), None)
        self._sync_out()
        code = int(status.item())
        if code:
            what = {1: "the section holds another type", 2: "the section's count is not outcount * Size()",
                    3: "the section passes the end of the image"}.get(code, "malformed section")
            raise MPIException(f"Unpack: {what} (status {code}) at position {position}")
        return pos.value

    # -- point-to-point (src/mpi/Comm.java:381-2460) on device tensors: counts in items of the datatype, offsets
    # in base elements. Multicore worlds (include/mpjx.h); host arrays are not routed.
    def _p2p_ptr(self, name, buf, offset, count, datatype):
        if buf is None and count == 0:
            return None
        if not _is_torch(buf):
            raise MPIException(f"{name} is provided for device-resident buffers")
        self._sync_in(buf)
        if datatype is MPI.PACKED:  # an image: a torch.uint8 tensor, offset and count in bytes
            if buf.dtype != _lib.torch.uint8:
                raise MPIException(f"{name}: an MPI.PACKED buffer must be a torch.uint8 tensor")
            return _dev_ptr(buf, offset, datatype, count)
        return _dev_ptr_dt(buf, offset, datatype, count)

    def Isend(self, buf, offset, count, datatype, dest, tag):
        p = self._p2p_ptr("Isend", buf, offset, count, datatype)
        h = ctypes.c_void_p()
        _wrap("mpjx_isend", self._h, p, count, datatype.code, dest, tag, ctypes.byref(h))
        return Request(self, h.value, buf)

    def Irecv(self, buf, offset, count, datatype, source, tag):
        p = self._p2p_ptr("Irecv", buf, offset, count, datatype)
        h = ctypes.c_void_p()
        _wrap("mpjx_irecv", self._h, p, count, datatype.code, source, tag, ctypes.byref(h))
        return Request(self, h.value, buf)

    def Send_init(self, buf, offset, count, datatype, dest, tag):
        """A persistent send (Comm.Send_init): checked now, posted by Prequest.Start / Startall."""
        p = self._p2p_ptr("Send_init", buf, offset, count, datatype)
        h = ctypes.c_void_p()
        _wrap("mpjx_send_init", self._h, p, count, datatype.code, dest, tag, ctypes.byref(h))
        return Prequest(self, h.value, buf)

    def Recv_init(self, buf, offset, count, datatype, source, tag):
        """A persistent receive (Comm.Recv_init)."""
        p = self._p2p_ptr("Recv_init", buf, offset, count, datatype)
        h = ctypes.c_void_p()
        _wrap("mpjx_recv_init", self._h, p, count, datatype.code, source, tag, ctypes.byref(h))
        return Prequest(self, h.value, buf)

    def Send(self, buf, offset, count, datatype, dest, tag):
        p = self._p2p_ptr("Send", buf, offset, count, datatype)
        _wrap("mpjx_send", self._h, p, count, datatype.code, dest, tag)

    def Recv(self, buf, offset, count, datatype, source, tag):
        p = self._p2p_ptr("Recv", buf, offset, count, datatype)
        st = _lib.Status()
        _wrap("mpjx_recv", self._h, p, count, datatype.code, source, tag, ctypes.byref(st))
        return Status(st)

    def Sendrecv(self, sendbuf, sendoffset, sendcount, sendtype, dest, sendtag, recvbuf, recvoffset, recvcount,
                 recvtype, source, recvtag):
        sp = self._p2p_ptr("Sendrecv", sendbuf, sendoffset, sendcount, sendtype)
        rp = self._p2p_ptr("Sendrecv", recvbuf, recvoffset, recvcount, recvtype)
        st = _lib.Status()
        _wrap("mpjx_sendrecv", self._h, sp, sendcount, sendtype.code, dest, sendtag, rp, recvcount, recvtype.code,
              source, recvtag, ctypes.byref(st))
        return Status(st)

    def Sendrecv_replace(self, buf, offset, count, datatype, dest, sendtag, source, recvtag):
        p = self._p2p_ptr("Sendrecv_replace", buf, offset, count, datatype)
        st = _lib.Status()
        _wrap("mpjx_sendrecv_replace", self._h, p, count, datatype.code, dest, sendtag, source, recvtag,
              ctypes.byref(st))
        return Status(st)

    def Iprobe(self, source, tag):
        """The Status of the first unmatched message a Recv(source, tag) posted now would take, or None
        (Comm.Iprobe). Nothing is consumed."""
        flag, st = ctypes.c_int(), _lib.Status()
        _wrap("mpjx_iprobe", self._h, source, tag, ctypes.byref(flag), ctypes.byref(st))
        return Status(st) if flag.value else None

    def Probe(self, source, tag):
        """Waits on the host for such a message and returns its Status (Comm.Probe)."""
        st = _lib.Status()
        _wrap("mpjx_probe", self._h, source, tag, ctypes.byref(st))
        return Status(st)

    def p2p_wire_stats(self):
        """(k_wire launches, pairs packed on the fly, pairs unpacked on the fly, pairs per launch) of this rank
        (mpjx_comm_p2p_wire_stats)."""
        a, b, c, m = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        _wrap("mpjx_comm_p2p_wire_stats", self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(m))
        return a.value, b.value, c.value, m.value

    def set_p2p_timeout(self, seconds):
        """This rank's limit on every point-to-point host wait (mpjx_comm_set_p2p_timeout)."""
        _wrap("mpjx_comm_set_p2p_timeout", self._h, float(seconds))

    def p2p_stats(self):
        """(launches, messages moved, eager sends, messages per launch) of this rank (mpjx_comm_p2p_stats)."""
        a, b, c, m = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        _wrap("mpjx_comm_p2p_stats", self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(m))
        return a.value, b.value, c.value, m.value

    def p2p_pool_stats(self):
        """(k_msgs_pool launches, segments stored, pairs moved from the pool, slots in use, pairs per launch) of
        this rank (mpjx_comm_p2p_pool_stats)."""
        a, b, c, d, m = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        _wrap("mpjx_comm_p2p_pool_stats", self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c), ctypes.byref(d),
              ctypes.byref(m))
        return a.value, b.value, c.value, d.value, m.value

    def Bcast(self, buf, offset, count, datatype, root):
        if not _is_torch(buf):
            raise MPIException("Bcast is provided for device-resident buffers")
        self._sync_in(buf)
        if datatype.derived:
            # the root sends to every other rank; its own entry stays empty (the same bytes on both sides)
            P, z, me = self._size, [0] * self._size, self._rank
            if me == root:
                return self._dt("Bcast", buf, offset, [0 if j == root else count for j in range(P)], z, datatype,
                                None, 0, z, z, datatype)
            return self._dt("Bcast", None, 0, z, z, datatype, buf, offset,
                            [count if j == root else 0 for j in range(P)], z, datatype)
        p = _dev_ptr(buf, offset, datatype, count)
        _wrap("mpjx_bcast", self._h, p, count, datatype.code, root, None)
        self._sync_out()


def _gs(fn, comm, sendbuf, sendoffset, sendcount, recvbuf, recvoffset, recvcount, datatype, root, send_all):
    if not (_is_torch(sendbuf) or _is_torch(recvbuf)):
        raise MPIException(f"{fn} is provided for device-resident buffers")
    if sendcount != recvcount:
        raise MPIException("sendcount must equal recvcount")
    comm._sync_in(*(b for b in (sendbuf, recvbuf) if b is not None))
    is_root = comm.Rank() == root
    if datatype.derived:  # block j of the root's side starts at j * count extents
        P, z = comm.Size(), [0] * comm.Size()
        blocks = [j * sendcount * datatype.extent for j in range(P)]
        one = [sendcount if j == root else 0 for j in range(P)]
        if send_all:
            return comm._dt("Scatter", sendbuf if is_root else None, sendoffset, [sendcount] * P if is_root else z,
                            blocks if is_root else z, datatype, recvbuf, recvoffset, one, z, datatype)
        return comm._dt("Gather", sendbuf, sendoffset, one, z, datatype, recvbuf if is_root else None, recvoffset,
                        [recvcount] * P if is_root else z, blocks if is_root else z, datatype)
    n_send = sendcount * (comm.Size() if (send_all and is_root) else 1)
    n_recv = recvcount * (comm.Size() if (not send_all and is_root) else 1)
    sp = _dev_ptr(sendbuf, sendoffset, datatype, n_send) if (is_root or not send_all) else None
    rp = _dev_ptr(recvbuf, recvoffset, datatype, n_recv) if (is_root or send_all) else None
    _wrap(fn, comm.handle, sp, rp, sendcount, datatype.code, root, None)
    comm._sync_out()


def Gather(comm, sendbuf, sendoffset, sendcount, recvbuf, recvoffset, recvcount, datatype, root):
    """Intracomm.Gather (src/mpi/PureIntracomm.java:782-1053) on device buffers, equal counts."""
    _gs("mpjx_gather", comm, sendbuf, sendoffset, sendcount, recvbuf, recvoffset, recvcount, datatype, root, False)


def Scatter(comm, sendbuf, sendoffset, sendcount, recvbuf, recvoffset, recvcount, datatype, root):
    """Intracomm.Scatter (src/mpi/PureIntracomm.java:1055-1171) on device buffers, equal counts."""
    _gs("mpjx_scatter", comm, sendbuf, sendoffset, sendcount, recvbuf, recvoffset, recvcount, datatype, root, True)


def combine(op, datatype, inout, inp, count=None, stream=None):
    """inout[i] = inp[i] (op) inout[i] on device tensors (one typed Op.perform)."""
    n = inout.numel() // datatype.size if count is None else count
    a = _dev_ptr(inout, 0, datatype, n)
    b = _dev_ptr(inp, 0, datatype, n)
    _wrap("mpjx_combine", op.opCode, datatype.code, a, b, n, stream)


def smp_world(nranks, devices=None, faithful=False):
    """Multicore mode: `nranks` ranks that are threads of this process (smpdev)."""
    devices = list(devices) if devices is not None else [0] * nranks
    arr = (ctypes.c_void_p * nranks)()
    devs = (ctypes.c_int * nranks)(*devices)
    _wrap("mpjx_comm_init_smp", arr, nranks, devs)
    comms = [Intracomm(arr[r], faithful=faithful) for r in range(nranks)]
    for c in comms:
        c._devices = list(devices)
    return comms


def run_multicore(comms, fn):
    """Run fn(comm) on one thread per rank, as MulticoreStarter does
    (src/runtime/starter/MulticoreStarter.java:309-322); returns per-rank results, re-raises errors."""
    out, err = [None] * len(comms), [None] * len(comms)

    def body(r):
        try:
            if _lib.torch is not None:
                _lib.torch.cuda.set_device(comms[r].device)
            out[r] = fn(comms[r])
        except BaseException as e:  # noqa: BLE001
            err[r] = e

    th = [threading.Thread(target=body, args=(r,)) for r in range(len(comms))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for e in err:
        if e is not None:
            raise e
    return out


def unique_id():
    buf = ctypes.create_string_buffer(128)
    _wrap("mpjx_get_unique_id", buf)
    return buf.raw


def Init(rank, size, device, uid):
    """One process per GPU over RCCL: every rank passes the same 128-byte unique id (from rank 0's
    unique_id(), shared out of band, e.g. torch.distributed.broadcast_object_list)."""
    h = ctypes.c_void_p()
    _wrap("mpjx_comm_init_rank", ctypes.byref(h), size, uid, rank, device)
    MPI.COMM_WORLD = Intracomm(h.value)
    MPI.COMM_WORLD._kind = "rccl"
    return MPI.COMM_WORLD


def InitIPC(rank, size, device, uid):
    """Processes of one node mapping each other's device buffers through HIP IPC (no RCCL): every
    rank passes the same 128-byte id (e.g. rank 0's unique_id(), or any bytes unique to the world)."""
    h = ctypes.c_void_p()
    _wrap("mpjx_comm_init_ipc", ctypes.byref(h), size, uid, rank, device)
    MPI.COMM_WORLD = Intracomm(h.value)
    MPI.COMM_WORLD._kind = "ipc"
    return MPI.COMM_WORLD
