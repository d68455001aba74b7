// mpjx.hpp — C++ host mirror of the reference's mpiJava-1.2 reduction API over the C ABI (mpjx.h).
//
// Same names, argument meaning and error behaviour as the Java classes on this path:
//   mpi::MPI::SUM / MPI::DOUBLE ...           src/mpi/MPI.java:117-126, src/mpi/Datatype.java:57-66
//   mpi::Intracomm::Reduce(sendbuf, sendoffset, recvbuf, recvoffset, count, datatype, op, root)
//                                            src/mpi/Intracomm.java:740-760
//   ::Allreduce / ::Reduce_scatter / ::Scan / ::Bcast / ::Barrier
//                                            src/mpi/Intracomm.java:787-885
//   ::Allgather / ::Allgatherv / ::Gatherv / ::Scatterv / ::Alltoall / ::Alltoallv (device pointers, sendtype
//   and recvtype as in mpiJava, of one base type)      src/mpi/Intracomm.java:363-690
//   mpi::Datatype::Contiguous / ::Vector      src/mpi/Contiguous.java, src/mpi/Vector.java: with a derived type
//   on either side (or two different types of one base type) the nine data-movement calls build the tables of
//   mpjx_alltoallv_dt: counts in items, v-call displacements in base elements, block j of an equal-count
//   call j * count extents into the buffer (mpjx.h)
//   ::Pack_size / ::Pack / ::Unpack          src/mpi/Comm.java:1860-1983: one mpjbuf section from, or into, items
//   of any datatype on a device buffer; the mpjbuf.Buffer is a pointer and a size (device or pinned host memory)
//   mpi::MPIException                       src/mpi/MPIException.java:42 (unchecked, like the Java one)
//   mpi::MPI::isOldSelected                  conf mpjexpress.mpi.old.collectives (src/mpi/MPI.java:70,266)
// Buffers are typed pointers; offsets and counts are in elements. Device pointers take the device
// path (blocking, like the Java calls); std::vector overloads are the host-resident path (the Java
// heap array case). Header-only: link libmpjx.
#pragma once
#include <mpjx.h>

#include <stdint.h>

#include <stdexcept>
#include <string>
#include <vector>

namespace mpi {

class MPIException : public std::runtime_error {
 public:
  explicit MPIException(const std::string& m) : std::runtime_error(m) {}
};

inline void check(int status, const char* what) {
  if (status != MPJX_SUCCESS)
    throw MPIException(std::string(what) + ": " + mpjx_strerror(status) + ": " + mpjx_last_error());
}

// A basic type, or a (value, index) pair type SHORT2..DOUBLE2 = Contiguous(2, base)
// (src/mpi/MPI.java:110-114): `code` crosses the C ABI; buffers are arrays of the base type,
// offsets are base-element indices, counts are datatype elements (pairs).
// A derived type (Contiguous, Vector, Hvector, Indexed, Hindexed, Struct) owns a code of the library's registry until Free(), as in mpiJava;
// copies share it.
struct Datatype {
  int code;
  int byteSize;  // bytes of the base type
  const char* name;
  int size = 1;      // base elements of data per item
  int extent = 0;    // base elements from one item to the next (0: size)
  int base = 0;      // the basic type's code (0: code & 0xff)
  bool derived = false;
  int lb = 0;        // the type's lb in base elements from an item's origin (mpjx_type_layout)
  int ub = 0;        // and its ub, from the library (made types only: `made`)
  bool made_ = false;  // extent, lb and ub are the library's, an extent of 0 included
  int Size() const { return size; }
  int Extent() const { return made_ ? extent : extent ? extent : size; }
  int Lb() const { return lb; }
  int Ub() const { return made_ ? ub : lb + Extent(); }
  int Base() const { return base ? base : (code & 0xff); }
  void Commit() const {}
  void Free() {
    if (!derived) return;
    check(mpjx_type_free(code), "Datatype.Free");
    derived = false;
  }
  static Datatype Contiguous(int count, const Datatype& oldtype) {
    int code = 0;
    check(mpjx_type_contiguous(count, oldtype.code, &code), "Datatype.Contiguous");
    return made(code, oldtype, "Contiguous");
  }
  static Datatype Vector(int count, int blocklength, int stride, const Datatype& oldtype) {
    int code = 0;
    check(mpjx_type_vector(count, blocklength, stride, oldtype.code, &code), "Datatype.Vector");
    return made(code, oldtype, "Vector");
  }
  // block j starts j * stride BASE elements from the origin; oldtype is any type (src/mpi/Hvector.java)
  static Datatype Hvector(int count, int blocklength, int stride, const Datatype& oldtype) {
    int code = 0;
    check(mpjx_type_hvector(count, blocklength, stride, oldtype.code, &code), "Datatype.Hvector");
    return made(code, oldtype, "Hvector");
  }
  // block i: blocklengths[i] items of oldtype from displacements[i] extents of oldtype (src/mpi/Indexed.java)
  static Datatype Indexed(const std::vector<int>& blocklengths, const std::vector<int>& displacements,
                          const Datatype& oldtype) {
    return indexed(mpjx_type_indexed, "Datatype.Indexed", blocklengths, displacements, oldtype);
  }
  // as Indexed, with displacements in BASE elements (src/mpi/Hindexed.java)
  static Datatype Hindexed(const std::vector<int>& blocklengths, const std::vector<int>& displacements,
                           const Datatype& oldtype) {
    return indexed(mpjx_type_hindexed, "Datatype.Hindexed", blocklengths, displacements, oldtype);
  }
  // block i: blocklengths[i] items of types[i] from displacements[i] BASE elements; MPI::LB and MPI::UB set the
  // bounds by the reference's order-dependent rules (src/mpi/Struct.java:149-386; include/mpjx.h)
  static Datatype Struct(const std::vector<int>& blocklengths, const std::vector<int>& displacements,
                         const std::vector<Datatype>& types) {
    if (blocklengths.size() != displacements.size() || blocklengths.size() != types.size())
      throw MPIException("Datatype.Struct: the three arrays differ in length");
    const std::vector<int64_t> b(blocklengths.begin(), blocklengths.end()), d(displacements.begin(), displacements.end());
    std::vector<int> codes;
    const Datatype* data = nullptr;
    for (const Datatype& t : types) {
      codes.push_back(t.code);
      if (!data && t.code != MPJX_LB && t.code != MPJX_UB) data = &t;
    }
    int code = 0;
    check(mpjx_type_struct((int)b.size(), b.data(), d.data(), codes.data(), &code), "Datatype.Struct");
    return made(code, data ? *data : Datatype{MPJX_BYTE, 1, "BYTE"}, "Struct");
  }
  static Datatype indexed(int (*fn)(int, const int64_t*, const int64_t*, int, int*), const char* name,
                          const std::vector<int>& bl, const std::vector<int>& ds, const Datatype& oldtype) {
    if (bl.size() != ds.size()) throw MPIException(std::string(name) + ": the two arrays differ in length");
    const std::vector<int64_t> b(bl.begin(), bl.end()), d(ds.begin(), ds.end());
    int code = 0;
    check(fn((int)b.size(), b.data(), d.data(), oldtype.code, &code), name);
    return made(code, oldtype, name);
  }
  // the Datatype of a code the library handed out
  static Datatype made(int code, const Datatype& oldtype, const char* name) {
    int base = 0;
    int64_t size = 0, extent = 0;
    int64_t lb = 0, ub = 0;
    check(mpjx_type_info(code, &base, &size, &extent), "mpjx_type_info");
    check(mpjx_type_layout(code, &lb, &ub, nullptr, nullptr), "mpjx_type_layout");
    if (size > INT32_MAX || ub > INT32_MAX || lb < INT32_MIN || extent > INT32_MAX) {
      (void)mpjx_type_free(code);
      throw MPIException(std::string(name) + ": the type exceeds this mirror's int sizes");
    }
    return Datatype{code, oldtype.byteSize, name, (int)size, (int)extent, base, true, (int)lb, (int)ub, true};
  }
};

struct Op {
  int opCode;
  const char* name;
};

struct MPI {
  static constexpr Datatype BYTE{MPJX_BYTE, 1, "BYTE"};
  static constexpr Datatype CHAR{MPJX_CHAR, 2, "CHAR"};
  static constexpr Datatype SHORT{MPJX_SHORT, 2, "SHORT"};
  static constexpr Datatype BOOLEAN{MPJX_BOOLEAN, 1, "BOOLEAN"};
  static constexpr Datatype INT{MPJX_INT, 4, "INT"};
  static constexpr Datatype LONG{MPJX_LONG, 8, "LONG"};
  static constexpr Datatype FLOAT{MPJX_FLOAT, 4, "FLOAT"};
  static constexpr Datatype DOUBLE{MPJX_DOUBLE, 8, "DOUBLE"};
  static constexpr Datatype SHORT2{MPJX_SHORT2, 2, "SHORT2", 2};
  static constexpr Datatype INT2{MPJX_INT2, 4, "INT2", 2};
  static constexpr Datatype LONG2{MPJX_LONG2, 8, "LONG2", 2};
  static constexpr Datatype FLOAT2{MPJX_FLOAT2, 4, "FLOAT2", 2};
  static constexpr Datatype DOUBLE2{MPJX_DOUBLE2, 8, "DOUBLE2", 2};
  static constexpr Datatype LB{MPJX_LB, 0, "LB", 0}, UB{MPJX_UB, 0, "UB", 0};  // components of Datatype::Struct only
  // an mpjbuf image, counted in bytes: the point-to-point calls only (include/mpjx.h "wire-format messages")
  static constexpr Datatype PACKED{MPJX_PACKED, 1, "PACKED"};
  static constexpr Op MAX{MPJX_MAX, "MAX"}, MIN{MPJX_MIN, "MIN"}, SUM{MPJX_SUM, "SUM"},
      PROD{MPJX_PROD, "PROD"}, LAND{MPJX_LAND, "LAND"}, BAND{MPJX_BAND, "BAND"}, LOR{MPJX_LOR, "LOR"},
      BOR{MPJX_BOR, "BOR"}, LXOR{MPJX_LXOR, "LXOR"}, BXOR{MPJX_BXOR, "BXOR"}, MAXLOC{MPJX_MAXLOC, "MAXLOC"},
      MINLOC{MPJX_MINLOC, "MINLOC"};
  static inline bool isOldSelected = false;
  static constexpr int ANY_SOURCE = MPJX_ANY_SOURCE, ANY_TAG = MPJX_ANY_TAG, PROC_NULL = MPJX_PROC_NULL,
                       UNDEFINED = MPJX_UNDEFINED;  // src/mpi/MPI.java:132-136
};

// mpi.Status (src/mpi/Status.java): source and tag of the matched message, and its length
struct Status {
  int source = MPJX_PROC_NULL, tag = MPJX_ANY_TAG;
  mpjx_status st{MPJX_PROC_NULL, MPJX_ANY_TAG, 0, 0, 0};
  Status() = default;
  explicit Status(const mpjx_status& s) : source(s.source), tag(s.tag), st(s) {}
  int Get_count(const Datatype& dt) const {
    int64_t c = 0;
    check(mpjx_get_count(&st, dt.code, &c, nullptr), "Get_count");
    return (int)c;
  }
  int Get_elements(const Datatype& dt) const {
    int64_t e = 0;
    check(mpjx_get_count(&st, dt.code, nullptr, &e), "Get_elements");
    return (int)e;
  }
  // bytes of the image a Recv(MPI::PACKED) of the probed message needs (mpjx_wire_bytes)
  int64_t wire_bytes() const {
    int64_t n = 0;
    check(mpjx_wire_bytes(&st, &n), "wire_bytes");
    return n;
  }
};

// mpi.Request (src/mpi/Request.java). The buffer belongs to the operation until Wait or a successful Test.
class Request {
 public:
  Request() = default;
  explicit Request(mpjx_request_t r) : r_(r) {}
  Request(const Request&) = delete;
  Request& operator=(const Request&) = delete;
  Request(Request&& o) noexcept : r_(o.r_) { o.r_ = nullptr; }
  Request& operator=(Request&& o) noexcept {
    if (this != &o) {
      Free();
      r_ = o.r_;
      o.r_ = nullptr;
    }
    return *this;
  }
  ~Request() { Free(); }
  bool Is_null() const { return r_ == nullptr; }
  Status Wait() {
    mpjx_status st;
    check(mpjx_wait(&r_, &st), "Wait");
    return Status(st);
  }
  // true (and *status set) if the operation is complete; never blocks
  bool Test(Status* status = nullptr) {
    mpjx_status st;
    int flag = 0;
    check(mpjx_test(&r_, &flag, &st), "Test");
    if (flag && status) *status = Status(st);
    return flag != 0;
  }
  void Free() {
    if (r_) mpjx_request_free(&r_);
  }
  // R: Request or Prequest. A Request is null afterwards; a Prequest stays, inactive.
  template <class R>
  static std::vector<Status> Waitall(std::vector<R>& reqs) {
    std::vector<mpjx_request_t> h;
    for (Request& r : reqs) h.push_back(r.r_);
    std::vector<mpjx_status> st(reqs.size() + 1);
    const int rc = mpjx_waitall((int)h.size(), h.data(), st.data());
    for (size_t i = 0; i < reqs.size(); i++) static_cast<Request&>(reqs[i]).r_ = h[i];
    check(rc, "Waitall");
    std::vector<Status> out;
    for (size_t i = 0; i < reqs.size(); i++) out.emplace_back(st[i]);
    return out;
  }

 protected:
  mpjx_request_t r_ = nullptr;
};

// mpi.Prequest (src/mpi/Prequest.java): a persistent request, made once by Intracomm::Send_init / Recv_init and
// activated by Start or Startall. Wait, Test and Waitall complete the activation and leave it non-null and
// inactive; Free() or the destructor releases it.
class Prequest : public Request {
 public:
  Prequest() = default;
  explicit Prequest(mpjx_request_t r) : Request(r) {}
  Prequest(Prequest&&) noexcept = default;
  Prequest& operator=(Prequest&&) noexcept = default;
  void Start() { check(mpjx_start(&r_), "Start"); }
  bool Is_active() const {
    int a = 0;
    check(mpjx_request_is_persistent(r_, nullptr, &a), "mpjx_request_is_persistent");
    return a != 0;
  }
  static void Startall(std::vector<Prequest>& reqs) {
    std::vector<mpjx_request_t> h;
    for (Prequest& r : reqs) h.push_back(r.r_);
    check(mpjx_startall((int)h.size(), h.data()), "Startall");
  }
};

// One rank's communicator (src/mpi/Intracomm.java). Not copyable; Free() or the destructor releases it.
class Intracomm {
 public:
  explicit Intracomm(mpjx_comm_t c, bool faithful = false) : c_(c), faithful_(faithful) {
    check(mpjx_comm_rank(c_, &rank_), "Rank");
    check(mpjx_comm_size(c_, &size_), "Size");
  }
  Intracomm(const Intracomm&) = delete;
  Intracomm& operator=(const Intracomm&) = delete;
  Intracomm(Intracomm&& o) noexcept : c_(o.c_), rank_(o.rank_), size_(o.size_), faithful_(o.faithful_) { o.c_ = nullptr; }
  ~Intracomm() { Free(); }

  int Rank() const { return rank_; }
  int Size() const { return size_; }
  mpjx_comm_t handle() const { return c_; }
  // the kernels this rank's last data-movement call launched: an OR of MPJX_MOVE_KERNEL_* (0: none)
  unsigned LastMoveKernels() const {
    unsigned m = 0;
    check(mpjx_comm_last_move_kernels(c_, &m), "mpjx_comm_last_move_kernels");
    return m;
  }
  void Free() {
    if (c_) mpjx_comm_destroy(c_);
    c_ = nullptr;
  }
  void Barrier() { check(mpjx_barrier(c_), "Barrier"); }

  // ---- point-to-point on device-resident buffers (src/mpi/Comm.java:381-2460): counts in items of the datatype,
  // offsets in base elements. Multicore worlds (include/mpjx.h).
  template <class T>
  Request Isend(const T* buf, int offset, int count, const Datatype& dt, int dest, int tag) {
    size_ok<T>(dt);
    mpjx_request_t r = nullptr;
    check(mpjx_isend(c_, buf ? buf + offset : nullptr, count, dt.code, dest, tag, &r), "Isend");
    return Request(r);
  }
  template <class T>
  Request Irecv(T* buf, int offset, int count, const Datatype& dt, int source, int tag) {
    size_ok<T>(dt);
    mpjx_request_t r = nullptr;
    check(mpjx_irecv(c_, buf ? buf + offset : nullptr, count, dt.code, source, tag, &r), "Irecv");
    return Request(r);
  }
  template <class T>
  Prequest Send_init(const T* buf, int offset, int count, const Datatype& dt, int dest, int tag) {
    size_ok<T>(dt);
    mpjx_request_t r = nullptr;
    check(mpjx_send_init(c_, buf ? buf + offset : nullptr, count, dt.code, dest, tag, &r), "Send_init");
    return Prequest(r);
  }
  template <class T>
  Prequest Recv_init(T* buf, int offset, int count, const Datatype& dt, int source, int tag) {
    size_ok<T>(dt);
    mpjx_request_t r = nullptr;
    check(mpjx_recv_init(c_, buf ? buf + offset : nullptr, count, dt.code, source, tag, &r), "Recv_init");
    return Prequest(r);
  }
  template <class T>
  void Send(const T* buf, int offset, int count, const Datatype& dt, int dest, int tag) {
    size_ok<T>(dt);
    check(mpjx_send(c_, buf ? buf + offset : nullptr, count, dt.code, dest, tag), "Send");
  }
  template <class T>
  Status Recv(T* buf, int offset, int count, const Datatype& dt, int source, int tag) {
    size_ok<T>(dt);
    mpjx_status st;
    check(mpjx_recv(c_, buf ? buf + offset : nullptr, count, dt.code, source, tag, &st), "Recv");
    return Status(st);
  }
  template <class T>
  Status Sendrecv(const T* sendbuf, int sendoffset, int sendcount, const Datatype& sendtype, int dest, int sendtag,
                  T* recvbuf, int recvoffset, int recvcount, const Datatype& recvtype, int source, int recvtag) {
    size_ok<T>(sendtype);
    size_ok<T>(recvtype);
    mpjx_status st;
    check(mpjx_sendrecv(c_, sendbuf ? sendbuf + sendoffset : nullptr, sendcount, sendtype.code, dest, sendtag,
                        recvbuf ? recvbuf + recvoffset : nullptr, recvcount, recvtype.code, source, recvtag, &st),
          "Sendrecv");
    return Status(st);
  }
  template <class T>
  Status Sendrecv_replace(T* buf, int offset, int count, const Datatype& dt, int dest, int sendtag, int source,
                          int recvtag) {
    size_ok<T>(dt);
    mpjx_status st;
    check(mpjx_sendrecv_replace(c_, buf ? buf + offset : nullptr, count, dt.code, dest, sendtag, source, recvtag, &st),
          "Sendrecv_replace");
    return Status(st);
  }
  // Comm.Iprobe: true and *status filled if a Recv(source, tag) posted now would take a message; nothing is consumed
  bool Iprobe(int source, int tag, Status* status = nullptr) {
    int flag = 0;
    mpjx_status st;
    check(mpjx_iprobe(c_, source, tag, &flag, &st), "Iprobe");
    if (flag && status) *status = Status(st);
    return flag != 0;
  }
  // Comm.Probe: waits on the host for such a message
  Status Probe(int source, int tag) {
    mpjx_status st;
    check(mpjx_probe(c_, source, tag, &st), "Probe");
    return Status(st);
  }
  void SetP2PTimeout(double seconds) { check(mpjx_comm_set_p2p_timeout(c_, seconds), "mpjx_comm_set_p2p_timeout"); }

  // ---- device-resident buffers (blocking) ----
  template <class T>
  void Reduce(const T* sendbuf, int sendoffset, T* recvbuf, int recvoffset, int count, const Datatype& dt,
              const Op& op, int root) {
    size_ok<T>(dt);
    // recvbuf: significant at the root; under faithful mode every rank's is written (MST partials)
    // a derived type: the reduction over its packed elements (mpjx_reduce_dt; recvbuf at the root only)
    check(dt.derived ? mpjx_reduce_dt(c_, sendbuf + sendoffset, rank_ == root ? recvbuf + recvoffset : nullptr, count,
                                      dt.code, op.opCode, root, flags(), nullptr)
                     : mpjx_reduce(c_, sendbuf + sendoffset,
                                   (rank_ == root || faithful_) ? recvbuf + recvoffset : nullptr, count, dt.code,
                                   op.opCode, root, flags(), nullptr),
          "Reduce");
    sync();
  }
  template <class T>
  void Allreduce(const T* sendbuf, int sendoffset, T* recvbuf, int recvoffset, int count, const Datatype& dt,
                 const Op& op) {
    size_ok<T>(dt);
    check((dt.derived ? mpjx_allreduce_dt : mpjx_allreduce)(c_, sendbuf + sendoffset, recvbuf + recvoffset, count, dt.code,
                                                            op.opCode, flags(), nullptr),
          "Allreduce");
    sync();
  }
  template <class T>
  void Reduce_scatter(const T* sendbuf, int sendoffset, T* recvbuf, int recvoffset, const std::vector<int>& recvcounts,
                      const Datatype& dt, const Op& op) {
    size_ok<T>(dt);
    std::vector<int64_t> rc = counts(recvcounts);
    check((dt.derived ? mpjx_reduce_scatter_dt : mpjx_reduce_scatter)(c_, sendbuf + sendoffset, recvbuf + recvoffset,
                                                                      rc.data(), dt.code, op.opCode, flags(), nullptr),
          "Reduce_scatter");
    sync();
  }
  template <class T>
  void Scan(const T* sendbuf, int sendoffset, T* recvbuf, int recvoffset, int count, const Datatype& dt, const Op& op) {
    size_ok<T>(dt);
    check((dt.derived ? mpjx_scan_dt : mpjx_scan)(c_, sendbuf + sendoffset, recvbuf + recvoffset, count, dt.code,
                                                  op.opCode, flags(), nullptr),
          "Scan");
    sync();
  }
  template <class T>
  void Bcast(T* buf, int offset, int count, const Datatype& dt, int root) {
    size_ok<T>(dt);
    if (dt.derived) {  // the root sends to every other rank; its own entry stays empty (the same bytes)
      std::vector<int64_t> z(size_, 0), sc(size_, rank_ == root ? count : 0), rc(size_, 0);
      sc[root] = 0;
      if (rank_ != root) rc[root] = count;
      return dt_move("Bcast", rank_ == root ? buf + offset : nullptr, sc, z, dt, rank_ == root ? nullptr : buf + offset,
                     rc, z, dt);
    }
    check(mpjx_bcast(c_, buf + offset, count, dt.code, root, nullptr), "Bcast");
    sync();
  }

  template <class T>
  void Gather(const T* sendbuf, int sendoffset, int sendcount, T* recvbuf, int recvoffset, int recvcount,
              const Datatype& dt, int root) {
    size_ok<T>(dt);
    if (sendcount != recvcount) throw MPIException("Gather: sendcount must equal recvcount");
    if (dt.derived) {
      std::vector<int64_t> z(size_, 0), sc(size_, 0), rc(size_, rank_ == root ? recvcount : 0);
      sc[root] = sendcount;
      return dt_move("Gather", sendbuf + sendoffset, sc, z, dt, rank_ == root ? recvbuf + recvoffset : nullptr, rc,
                     rank_ == root ? blocks(recvcount, dt) : z, dt);
    }
    check(mpjx_gather(c_, sendbuf + sendoffset, rank_ == root ? recvbuf + recvoffset : nullptr, sendcount, dt.code,
                      root, nullptr),
          "Gather");
    sync();
  }
  template <class T>
  void Scatter(const T* sendbuf, int sendoffset, int sendcount, T* recvbuf, int recvoffset, int recvcount,
               const Datatype& dt, int root) {
    size_ok<T>(dt);
    if (sendcount != recvcount) throw MPIException("Scatter: sendcount must equal recvcount");
    if (dt.derived) {
      std::vector<int64_t> z(size_, 0), sc(size_, rank_ == root ? sendcount : 0), rc(size_, 0);
      rc[root] = recvcount;
      return dt_move("Scatter", rank_ == root ? sendbuf + sendoffset : nullptr, sc,
                     rank_ == root ? blocks(sendcount, dt) : z, dt, recvbuf + recvoffset, rc, z, dt);
    }
    check(mpjx_scatter(c_, rank_ == root ? sendbuf + sendoffset : nullptr, recvbuf + recvoffset, recvcount, dt.code,
                       root, nullptr),
          "Scatter");
    sync();
  }

  // ---- block moves on device buffers (src/mpi/Intracomm.java:363-690): counts, displacements and
  // offsets in elements; count tables significant where MPI says (mpjx.h) ----
  template <class T>
  void Allgather(const T* sendbuf, int sendoffset, int sendcount, const Datatype& sendtype, T* recvbuf,
                 int recvoffset, int recvcount, const Datatype& recvtype) {
    if (strided<T>(sendtype, recvtype, "Allgather")) {
      equal_length("Allgather", sendcount, sendtype, recvcount, recvtype);
      return dt_move("Allgather", sendbuf + sendoffset, std::vector<int64_t>(size_, sendcount),
                     std::vector<int64_t>(size_, 0), sendtype, recvbuf + recvoffset,
                     std::vector<int64_t>(size_, recvcount), blocks(recvcount, recvtype), recvtype);
    }
    if (sendcount != recvcount) throw MPIException("Allgather: sendcount must equal recvcount");
    check(mpjx_allgather(c_, sendbuf + sendoffset, recvbuf + recvoffset, sendcount, sendtype.code, nullptr),
          "Allgather");
    sync();
  }
  template <class T>
  void Allgatherv(const T* sendbuf, int sendoffset, int sendcount, const Datatype& sendtype, T* recvbuf,
                  int recvoffset, const std::vector<int>& recvcount, const std::vector<int>& displs,
                  const Datatype& recvtype) {
    std::vector<int64_t> rc = counts(recvcount), rd = counts(displs);
    if (strided<T>(sendtype, recvtype, "Allgatherv"))
      return dt_move("Allgatherv", sendbuf + sendoffset, std::vector<int64_t>(size_, sendcount),
                     std::vector<int64_t>(size_, 0), sendtype, recvbuf + recvoffset, rc, rd, recvtype);
    check(mpjx_allgatherv(c_, sendbuf + sendoffset, sendcount, recvbuf + recvoffset, rc.data(), rd.data(),
                          sendtype.code, nullptr),
          "Allgatherv");
    sync();
  }
  template <class T>
  void Gatherv(const T* sendbuf, int sendoffset, int sendcount, const Datatype& sendtype, T* recvbuf,
               int recvoffset, const std::vector<int>& recvcount, const std::vector<int>& displs,
               const Datatype& recvtype, int root) {
    std::vector<int64_t> rc, rd;
    if (rank_ == root) {
      rc = counts(recvcount);
      rd = counts(displs);
    }
    if (strided<T>(sendtype, recvtype, "Gatherv")) {
      std::vector<int64_t> z(size_, 0), sc(size_, 0);
      sc[root] = sendcount;
      return dt_move("Gatherv", sendbuf + sendoffset, sc, z, sendtype, rank_ == root ? recvbuf + recvoffset : nullptr,
                     rank_ == root ? rc : z, rank_ == root ? rd : z, recvtype);
    }
    check(mpjx_gatherv(c_, sendbuf + sendoffset, sendcount, rank_ == root ? recvbuf + recvoffset : nullptr,
                       rank_ == root ? rc.data() : nullptr, rank_ == root ? rd.data() : nullptr, sendtype.code, root,
                       nullptr),
          "Gatherv");
    sync();
  }
  template <class T>
  void Scatterv(const T* sendbuf, int sendoffset, const std::vector<int>& sendcount, const std::vector<int>& displs,
                const Datatype& sendtype, T* recvbuf, int recvoffset, int recvcount, const Datatype& recvtype,
                int root) {
    std::vector<int64_t> sc, sd;
    if (rank_ == root) {
      sc = counts(sendcount);
      sd = counts(displs);
    }
    if (strided<T>(sendtype, recvtype, "Scatterv")) {
      std::vector<int64_t> z(size_, 0), rc(size_, 0);
      rc[root] = recvcount;
      return dt_move("Scatterv", rank_ == root ? sendbuf + sendoffset : nullptr, rank_ == root ? sc : z,
                     rank_ == root ? sd : z, sendtype, recvbuf + recvoffset, rc, z, recvtype);
    }
    check(mpjx_scatterv(c_, rank_ == root ? sendbuf + sendoffset : nullptr, rank_ == root ? sc.data() : nullptr,
                        rank_ == root ? sd.data() : nullptr, recvbuf + recvoffset, recvcount, sendtype.code, root,
                        nullptr),
          "Scatterv");
    sync();
  }
  template <class T>
  void Alltoall(const T* sendbuf, int sendoffset, int sendcount, const Datatype& sendtype, T* recvbuf,
                int recvoffset, int recvcount, const Datatype& recvtype) {
    if (strided<T>(sendtype, recvtype, "Alltoall")) {
      equal_length("Alltoall", sendcount, sendtype, recvcount, recvtype);
      return dt_move("Alltoall", sendbuf + sendoffset, std::vector<int64_t>(size_, sendcount),
                     blocks(sendcount, sendtype), sendtype, recvbuf + recvoffset,
                     std::vector<int64_t>(size_, recvcount), blocks(recvcount, recvtype), recvtype);
    }
    if (sendcount != recvcount) throw MPIException("Alltoall: sendcount must equal recvcount");
    check(mpjx_alltoall(c_, sendbuf + sendoffset, recvbuf + recvoffset, sendcount, sendtype.code, nullptr),
          "Alltoall");
    sync();
  }
  template <class T>
  void Alltoallv(const T* sendbuf, int sendoffset, const std::vector<int>& sendcount,
                 const std::vector<int>& sdispls, const Datatype& sendtype, T* recvbuf, int recvoffset,
                 const std::vector<int>& recvcount, const std::vector<int>& rdispls, const Datatype& recvtype) {
    std::vector<int64_t> sc = counts(sendcount), sd = counts(sdispls), rc = counts(recvcount), rd = counts(rdispls);
    if (strided<T>(sendtype, recvtype, "Alltoallv"))
      return dt_move("Alltoallv", sendbuf + sendoffset, sc, sd, sendtype, recvbuf + recvoffset, rc, rd, recvtype);
    check(mpjx_alltoallv(c_, sendbuf + sendoffset, sc.data(), sd.data(), recvbuf + recvoffset, rc.data(), rd.data(),
                         sendtype.code, nullptr),
          "Alltoallv");
    sync();
  }

  // ---- Pack / Unpack / Pack_size (src/mpi/Comm.java:1860-1983): one mpjbuf section from, or into, items of
  // any datatype on a device buffer. The image (mpjbuf.Buffer there) is `bytes` bytes of device or pinned host
  // memory; positions are bytes; the new position is returned. Local calls (mpjx.h) ----
  int64_t Pack_size(int incount, const Datatype& dt) const {
    int64_t n = 0;
    check(mpjx_pack_size(incount, dt.code, &n), "Pack_size");
    return n;
  }
  template <class T>
  int64_t Pack(const T* inbuf, int offset, int incount, const Datatype& dt, void* outbuf, int64_t bytes,
               int64_t position) {
    size_ok<T>(dt);
    check(mpjx_pack(c_, inbuf + offset, incount, dt.code, outbuf, bytes, &position, nullptr), "Pack");
    sync();
    return position;
  }
  // a section of another type or count, or one that passes the end of the image, throws and leaves outbuf untouched
  template <class T>
  int64_t Unpack(const void* inbuf, int64_t bytes, int64_t position, T* outbuf, int offset, int outcount,
                 const Datatype& dt) {
    size_ok<T>(dt);
    void* st = nullptr;  // the kernel's status word: pinned, so the host reads it after the call
    check(mpjx_host_alloc(&st, sizeof(int)), "Unpack");
    *(volatile int*)st = 0;
    int rc = mpjx_unpack(c_, inbuf, bytes, &position, outbuf + offset, outcount, dt.code, (int*)st, nullptr);
    if (rc == MPJX_SUCCESS) rc = mpjx_comm_synchronize(c_);
    const int code = *(volatile int*)st;
    (void)mpjx_host_free(st);
    check(rc, "Unpack");
    if (code) throw MPIException("Unpack: malformed section (status " + std::to_string(code) + ")");
    return position;
  }

  // ---- host-resident arrays (the Java heap array case) ----
  template <class T>
  void Reduce(const std::vector<T>& sendbuf, int sendoffset, std::vector<T>& recvbuf, int recvoffset, int count,
              const Datatype& dt, const Op& op, int root) {
    size_ok<T>(dt);
    no_host_dt(dt, "Reduce");
    extent(sendbuf, sendoffset, count, dt.Size());
    const bool all_recv = rank_ == root || faithful_;  // faithful: every rank's recvbuf is written
    if (all_recv) extent(recvbuf, recvoffset, count, dt.Size());
    check(mpjx_reduce_host(c_, sendbuf.data() + sendoffset, all_recv ? recvbuf.data() + recvoffset : nullptr,
                           count, dt.code, op.opCode, root, flags()),
          "Reduce");
  }
  template <class T>
  void Allreduce(const std::vector<T>& sendbuf, int sendoffset, std::vector<T>& recvbuf, int recvoffset, int count,
                 const Datatype& dt, const Op& op) {
    size_ok<T>(dt);
    no_host_dt(dt, "Allreduce");
    extent(sendbuf, sendoffset, count, dt.Size());
    extent(recvbuf, recvoffset, count, dt.Size());
    check(mpjx_allreduce_host(c_, sendbuf.data() + sendoffset, recvbuf.data() + recvoffset, count, dt.code,
                              op.opCode, flags()),
          "Allreduce");
  }
  template <class T>
  void Reduce_scatter(const std::vector<T>& sendbuf, int sendoffset, std::vector<T>& recvbuf, int recvoffset,
                      const std::vector<int>& recvcounts, const Datatype& dt, const Op& op) {
    size_ok<T>(dt);
    no_host_dt(dt, "Reduce_scatter");
    std::vector<int64_t> rc = counts(recvcounts);
    int64_t total = 0;
    for (int64_t x : rc) total += x;
    extent(sendbuf, sendoffset, total, dt.Size());
    extent(recvbuf, recvoffset, rc[rank_], dt.Size());
    check(mpjx_reduce_scatter_host(c_, sendbuf.data() + sendoffset, recvbuf.data() + recvoffset, rc.data(),
                                   dt.code, op.opCode, flags()),
          "Reduce_scatter");
  }
  template <class T>
  void Scan(const std::vector<T>& sendbuf, int sendoffset, std::vector<T>& recvbuf, int recvoffset, int count,
            const Datatype& dt, const Op& op) {
    size_ok<T>(dt);
    no_host_dt(dt, "Scan");
    extent(sendbuf, sendoffset, count, dt.Size());
    extent(recvbuf, recvoffset, count, dt.Size());
    check(mpjx_scan_host(c_, sendbuf.data() + sendoffset, recvbuf.data() + recvoffset, count, dt.code,
                         op.opCode, flags()),
          "Scan");
  }

 private:
  // the *_host variants take basic and pair types: a derived type reduces device-resident buffers only
  static void no_host_dt(const Datatype& dt, const char* what) {
    if (dt.derived) throw MPIException(std::string(what) + ": a derived datatype is provided for device-resident buffers");
  }
  // the mpiJava calls are blocking: every call returns complete (MPJX_FLAG_BLOCKING)
  unsigned flags() const {
    return (MPI::isOldSelected ? MPJX_FLAG_OLD_COLLECTIVES : 0u) | (faithful_ ? MPJX_FLAG_FAITHFUL : 0u) |
           MPJX_FLAG_BLOCKING;
  }
  void sync() { check(mpjx_comm_synchronize(c_), "synchronize"); }
  template <class T>
  static void size_ok(const Datatype& dt) {
    if ((int)sizeof(T) != dt.byteSize)
      throw MPIException(std::string("buffer element size does not match MPI.") + dt.name);
  }
  // True if the call takes the strided path (mpjx_alltoallv_dt): a derived type on either side, or two
  // different types of one base type. Two equal basic or pair types take the path they always took.
  template <class T>
  static bool strided(const Datatype& sendtype, const Datatype& recvtype, const char* what) {
    if (sendtype.Base() != recvtype.Base())
      throw MPIException(std::string(what) + ": sendtype differs from recvtype in its base type");
    size_ok<T>(sendtype);
    return sendtype.derived || recvtype.derived || sendtype.code != recvtype.code;
  }
  static void equal_length(const char* what, int sendcount, const Datatype& st, int recvcount, const Datatype& rt) {
    if ((int64_t)sendcount * st.Size() != (int64_t)recvcount * rt.Size())
      throw MPIException(std::string(what) + ": the send and receive lengths differ");
  }
  // Block j of an equal-count call: j * count extents into the buffer, in base elements
  std::vector<int64_t> blocks(int count, const Datatype& dt) const {
    std::vector<int64_t> d(size_);
    for (int j = 0; j < size_; j++) d[j] = (int64_t)j * count * dt.Extent();
    return d;
  }
  void dt_move(const char* what, const void* sendbuf, const std::vector<int64_t>& sc, const std::vector<int64_t>& sd,
               const Datatype& st, void* recvbuf, const std::vector<int64_t>& rc, const std::vector<int64_t>& rd,
               const Datatype& rt) {
    check(mpjx_alltoallv_dt(c_, sendbuf, sc.data(), sd.data(), st.code, recvbuf, rc.data(), rd.data(), rt.code, nullptr),
          what);
    sync();
  }
  template <class T>
  static void extent(const std::vector<T>& v, int off, int64_t count, int size = 1) {
    if (off < 0 || count < 0 || (int64_t)off + count * size > (int64_t)v.size())
      throw MPIException("offset + count exceeds the array length");
  }
  std::vector<int64_t> counts(const std::vector<int>& rc) const {
    if ((int)rc.size() < size_) throw MPIException("recvcounts shorter than the communicator");
    return std::vector<int64_t>(rc.begin(), rc.begin() + size_);
  }

  mpjx_comm_t c_;
  int rank_ = 0, size_ = 1;
  bool faithful_;
};

// Multicore mode (smpdev): nranks ranks that are threads of this process, all on `devices`.
inline std::vector<Intracomm> smp_world(int nranks, const std::vector<int>& devices) {
  std::vector<mpjx_comm_t> h(nranks);
  check(mpjx_comm_init_smp(h.data(), nranks, devices.data()), "mpjx_comm_init_smp");
  std::vector<Intracomm> w;
  w.reserve(nranks);
  for (mpjx_comm_t c : h) w.emplace_back(c);
  return w;
}

// One process per GPU over RCCL (MPJDev.init + COMM_WORLD, src/mpi/MPI.java:298-305): every rank
// passes the id rank 0 got from mpjx_get_unique_id, shared out of band.
inline Intracomm Init(int rank, int size, int device, const mpjx_unique_id& id) {
  mpjx_comm_t c = nullptr;
  check(mpjx_comm_init_rank(&c, size, &id, rank, device), "mpjx_comm_init_rank");
  return Intracomm(c);
}

// Processes of one node without RCCL: the HIP-IPC direct engine (id: any bytes unique to the world).
inline Intracomm InitIPC(int rank, int size, int device, const mpjx_unique_id& id) {
  mpjx_comm_t c = nullptr;
  check(mpjx_comm_init_ipc(&c, size, &id, rank, device), "mpjx_comm_init_ipc");
  return Intracomm(c);
}

// Multicore mode, formed by the rank threads themselves (each thread calls this for its rank with the
// world's id and all ranks' devices; one world per communicator, as Split/Create need).
inline Intracomm InitSMPRank(int rank, int size, const std::vector<int>& devices, const mpjx_unique_id& id) {
  mpjx_comm_t c = nullptr;
  check(mpjx_comm_init_smp_rank(&c, size, &id, rank, devices.data()), "mpjx_comm_init_smp_rank");
  return Intracomm(c);
}

}  // namespace mpi
