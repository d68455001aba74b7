/*
 * mpjx.h — C ABI of libmpjx, the MI355X-native (gfx950) reduction-collective path of MPJ Express.
 *
 * Drop-in boundary. The reference routes Reduce/Allreduce/Reduce_scatter/Scan through an
 * IntracommImpl strategy (src/mpi/IntracommImpl.java:426-503, chosen at src/mpi/Intracomm.java:63-67);
 * its only native reduction is the JNI entry point
 *   Java_mpjdev_natmpjdev_Intracomm_nativeReduce(JNIEnv*, jobject, jlong comm, jobject sendArray,
 *       jobject recvDirectBuffer, jint count, jint type, jint op, jint root)
 *   (src/mpjdev/natmpjdev/lib/mpjdev_natmpjdev_Intracomm.c:410-627, bound at
 *    src/mpjdev/natmpjdev/Intracomm.java:723-737)
 * which hands `type.baseType` and `op.opCode` to MPI_Reduce. Every entry point below takes those
 * same integer codes unchanged, plain pointers and 64-bit element counts; nothing here mentions
 * torch, JNI or Java types. INTEGRATION.md shows the JNI shim and the HipIntracomm class a
 * maintainer adds on the Java side.
 *
 * Conventions
 *  - Every function returns an int status: MPJX_SUCCESS (0) or a negative MPJX_ERR_* code;
 *    mpjx_strerror() names it and mpjx_last_error() gives the calling thread's detail message
 *    (the reference throws mpi.MPIException: src/mpi/MPIException.java:42).
 *  - Device-pointer entry points ENQUEUE work on `stream` (a hipStream_t passed as void*; NULL =
 *    the communicator's own stream) and return without waiting; mpjx_comm_synchronize() waits.
 *    Consecutive calls on one communicator are ordered: a call on another stream than the previous
 *    call's waits for that stream, so the previous call's stream must stay valid until then (or
 *    until mpjx_comm_synchronize / mpjx_comm_destroy).
 *  - Element semantics are the reference's typed Op bodies (acc[i] = in[i] (op) acc[i]) with Java
 *    arithmetic: integer wrap-around, char unsigned, MAX/MIN as `if (in > acc) acc = in`
 *    (NaN never replaces, +0/-0 ties keep the accumulator), IEEE float/double with subnormals.
 *  - Combine ORDER follows the reference algorithm selected by `flags`, so float/double results
 *    are bit-identical to the reference's pure-Java collectives on the same inputs.
 *  - Device entry points check that every buffer is GPU-accessible (device, managed, or host memory
 *    allocated with hipHostMalloc) before any kernel runs, and return MPJX_ERR_ARG otherwise.
 *  - A collective call that fails on a rank (rejected arguments, a bad root, a failed step part-way)
 *    marks multicore and IPC worlds failed: the other ranks' matching and later calls return
 *    MPJX_ERR_INTERNAL instead of waiting for it (destroy and re-create the communicator). In RCCL
 *    worlds the other ranks wait, as MPI ranks do (MPJX_RCCL_TIMEOUT_S ends the wait), and at P > 1
 *    the failing rank's communicator is aborted: its later calls return MPJX_ERR_RCCL instead of
 *    pairing with the peers' pending operation.
 *  - The caller owns every buffer; the library owns streams, events and device scratch, cached
 *    per communicator. Calls on one communicator must come from one thread at a time (MPI
 *    semantics); several communicators may be driven concurrently from different threads.
 */
#ifndef MPJX_H
#define MPJX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPJX_VERSION 100 /* 1.0.0 */

/* mpi.Datatype.baseType codes (src/mpi/Datatype.java:57-66); byte sizes src/mpi/BasicType.java:50-140 */
enum {
  MPJX_BYTE = 1,    /* Java byte,    int8  */
  MPJX_CHAR = 2,    /* Java char,    uint16 */
  MPJX_SHORT = 3,   /* Java short,   int16 */
  MPJX_BOOLEAN = 4, /* Java boolean, uint8 0/1 */
  MPJX_INT = 5,     /* Java int,     int32 */
  MPJX_LONG = 6,    /* Java long,    int64 */
  MPJX_FLOAT = 7,   /* Java float,   IEEE binary32 */
  MPJX_DOUBLE = 8   /* Java double,  IEEE binary64 */
};

/* (value, index) pair types MPI.SHORT2/INT2/LONG2/FLOAT2/DOUBLE2 = Datatype.Contiguous(2, base)
 * (src/mpi/MPI.java:110-114): code = 0x100 | base code; one element = one pair; only MAXLOC/MINLOC. */
enum {
  MPJX_SHORT2 = 0x103, MPJX_INT2 = 0x105, MPJX_LONG2 = 0x106, MPJX_FLOAT2 = 0x107, MPJX_DOUBLE2 = 0x108
};

/* The bound markers MPI.LB / MPI.UB (src/mpi/Datatype.java:68-69; BasicType.java:145-170): no base type, size
 * 0, lb = ub = 0 with lbSet (LB) or ubSet (UB). Valid only as a component of mpjx_type_struct; every other entry
 * point returns MPJX_ERR_ARG for them (an unknown datatype code). */
enum { MPJX_LB = 10, MPJX_UB = 11 };

/* MPI.PACKED (src/mpi/MPI.java:96, Datatype.java:67): an mpjbuf image, counted in BYTES. Valid only in the
 * point-to-point calls named under "wire-format messages" below; mpjx_type_size(9) is 0 and every other entry
 * point returns MPJX_ERR_ARG for it (an unknown datatype code). */
enum { MPJX_PACKED = 9 };

/* mpi.Op.opCode values (src/mpjdev/Constants.java:53-64; MPI.MAX..MPI.MINLOC at src/mpi/MPI.java:117-130) */
enum {
  MPJX_MAX = 1, MPJX_MIN = 2, MPJX_SUM = 3, MPJX_PROD = 4, MPJX_LAND = 5,
  MPJX_BAND = 6, MPJX_LOR = 7, MPJX_BOR = 8, MPJX_LXOR = 9, MPJX_BXOR = 10,
  MPJX_MAXLOC = 11, /* src/mpi/Maxloc.java: larger value wins; equal values keep the smaller index */
  MPJX_MINLOC = 12  /* src/mpi/Minloc.java: smaller value wins; equal values keep the smaller index */
};

/* status codes */
enum {
  MPJX_SUCCESS = 0,
  MPJX_ERR_ARG = -1,         /* bad pointer/count/rank/root argument */
  MPJX_ERR_OP_TYPE = -2,     /* the reference's *Worker.getWorker throws for this (op, type) */
  MPJX_ERR_HIP = -3,         /* HIP runtime error */
  MPJX_ERR_RCCL = -4,        /* RCCL error */
  MPJX_ERR_NO_DEVICE = -5,   /* no usable gfx950 device / kernel image */
  MPJX_ERR_UNSUPPORTED = -6, /* combination not provided by this build */
  MPJX_ERR_INTERNAL = -7
};

/* flags (collectives) */
#define MPJX_FLAG_OLD_COLLECTIVES 0x1u /* mirror conf `mpjexpress.mpi.old.collectives=true`
                                          (MPI.isOldSelected, src/mpi/MPI.java:70,266): flat-tree
                                          orders of FT_Reduce / FT_Allreduce / FT_Reduce_scatter */
#define MPJX_FLAG_FAITHFUL 0x2u        /* reproduce the reference's observable state, defects
                                          included. Results: BOR/BXOR never combine (every perform
                                          keeps the accumulator; src/mpi/BorInt.java:50 overloads
                                          instead of overriding src/mpi/Op.java:56); the P>=3 bucket
                                          Reduce_scatter result (src/mpi/PureIntracomm.java:2377-2439).
                                          Buffers written BEYOND the MPI contract (see each call):
                                          - mpjx_reduce, default order: EVERY rank's recvbuf (count
                                            elements) = the MST reduction of the largest sub-tree the
                                            rank roots (:1937-1939 copy send into recvbuf and reduce
                                            there); the root's is the result;
                                          - mpjx_reduce, with MPJX_FLAG_OLD_COLLECTIVES: every
                                            non-root's recvbuf = a copy of its sendbuf (:2038,2052);
                                          - mpjx_reduce_scatter, default order, P>=2, non-pair types:
                                            the caller's SENDBUF is overwritten (:2427-2428): its own
                                            block (at sum(recvcounts[0..rank))) = the rank's result,
                                            every other element x = x (op) 0 folded P-1 times.
                                          Not reproduced: the nonzero-offset loop-bound quirk (no
                                          offsets cross this ABI) and FT_Reduce_scatter's full-length
                                          recvbuf writes (the Java strategy keeps those calls,
                                          INTEGRATION.md). */

#define MPJX_FLAG_SEND_BIG_ENDIAN 0x4u /* sendbuf elements are big-endian: an mpjbuf section payload as
                                          niodev delivers it (src/mpjbuf/NIOBuffer.java:42, encoding
                                          never changed, src/mpjbuf/Buffer.java:5414) */
#define MPJX_FLAG_RECV_BIG_ENDIAN 0x8u /* write recvbuf big-endian (ready to send on as mpjbuf) */
#define MPJX_FLAG_BLOCKING 0x10u       /* return only once the call's results are complete, as if followed by
                                          mpjx_comm_synchronize (the mpiJava calls are blocking:
                                          src/mpi/Intracomm.java:740-885). In multicore mode the ranks then
                                          end a call with a host rendezvous after the launching rank's
                                          stream has drained, instead of ordering every rank's stream after
                                          it by events. Ignored by the *_host variants (synchronous anyway). */
/* Both byte-order flags are part of the call's datatype: pass the same ones on every rank, like
 * `type` and `op`. The combine kernels swap in registers (no extra pass over the vector). */

typedef struct mpjx_comm *mpjx_comm_t;
typedef struct {
  char internal[128]; /* == ncclUniqueId */
} mpjx_unique_id;

/* ---- library ------------------------------------------------------------------------------- */
int mpjx_version(void);
/* The HIP runtime and RCCL versions this process actually bound (not the headers it was built
 * against: a JVM binds /opt/rocm's, a Python process the ones torch loaded first). Either pointer may
 * be NULL. MPJX_ERR_HIP if the HIP runtime does not answer. */
int mpjx_runtime_versions(int *hip_runtime, int *rccl);
const char *mpjx_strerror(int status);
const char *mpjx_last_error(void); /* detail of the calling thread's last failure */
/* Bytes per element of a datatype code, 0 if unknown (BasicType.byteSize). */
int mpjx_type_size(int type);
/* MPJX_SUCCESS if the reference has a typed worker for (op, type), else MPJX_ERR_OP_TYPE
 * (e.g. SUM on BOOLEAN: src/mpi/SumWorker.java:60; BAND on DOUBLE: src/mpi/BandWorker.java:60). */
int mpjx_op_check(int op, int type);
/* Number of visible devices that this build can run on (gfx950). */
int mpjx_device_count(int *count);

/* ---- element-wise combine (the typed Op.perform loop, src/mpi/SumDouble.java:49-55) --------- */
/* inout[i] = in[i] (op) inout[i], i in [0, count), device pointers. Replaces one
 * createInitialBuffer/perform/getResultant round trip (src/mpi/PureIntracomm.java:1979-1986). */
int mpjx_combine(int op, int type, void *inout, const void *in, int64_t count, void *stream);

/* P-way combine in a reference ORDER: the local reduction step that follows an exchange (the
 * reference performs it edge by edge inside MST_Reduce / FT_Reduce / Scan). `in[0..P)` are P
 * operand slices of `count` elements (index = rank); out[0] receives the result slice, or for
 * MPJX_ORDER_SCAN out[0..P) receive every rank's inclusive prefix. Device pointers; an output may
 * alias an input.
 *   MPJX_ORDER_MST   out[0] = MST_Reduce tree over ranks 0..P-1 rooted at `root` (PureIntracomm.java:1943-1992)
 *   MPJX_ORDER_FOLD  out[0] = in[P-1] (op) (... (op) (in[1] (op) in[0]))  (FT_Reduce with in[0] = x_root)
 *   MPJX_ORDER_SCAN  out[r] = in[r-1] (op) (... (op) (in[0] (op) in[r]))   (Scan, :2526-2544)        */
enum { MPJX_ORDER_FOLD = 0, MPJX_ORDER_MST = 1, MPJX_ORDER_SCAN = 2 };
int mpjx_combine_multi(int op, int type, int order, int P, const void *const *in, void *const *out,
                       int64_t count, int root, unsigned flags, void *stream);

/* mpjbuf section header at byte `pos` (rounded up to the 8-byte ALIGNMENT_UNIT) of a static buffer
 * of `nbytes` (src/mpjbuf/Buffer.java:609-704 putSectionHeader/getSectionHeader: type code byte,
 * big-endian int32 element count at +4, payload at +8 = SECTION_OVERHEAD). Returns the datatype
 * code (mpjbuf.Type code + 1 for the 8 basic types, src/mpjbuf/Type.java:66-73), the element count
 * and the payload's byte position, so a caller can reduce a niodev payload in place with the
 * BIG_ENDIAN flags instead of unpacking it on the host. Host memory only; no device work. */
int mpjx_mpjbuf_section(const void *buf, int64_t nbytes, int64_t pos, int *type, int64_t *count,
                        int64_t *data_pos);

/* The per-edge combine of MST_Reduce on a packed message, with the section walk on the device:
 * acc[i] = payload[i] (op) acc[i] for i < count, where the payload is the big-endian element run of
 * the mpjbuf sections at the start of `msg` (a static-buffer image of msg_bytes bytes, e.g. a niodev
 * message in device memory or in pinned host memory; src/mpjbuf/Buffer.java:609-704 section headers,
 * NIOBuffer.java:520-563 big-endian elements; a message may hold several sections of the type, read
 * in order; pair types are sections of their base type). Replaces the host unpack + perform of
 * PureIntracomm.java:1979-1986 with one HBM pass. The kernel reads the headers: a wrong type code
 * (1), element counts that do not add up to count (2), a header or payload past msg_bytes (3) or more
 * than 64 sections (4) leave acc untouched and store that code into *status (a device-accessible int
 * the caller zeroes); 0 stays there on success. Asynchronous on `stream`. flags: MPJX_FLAG_FAITHFUL
 * only. */
#define MPJX_MPJBUF_BAD_TYPE 1
#define MPJX_MPJBUF_BAD_COUNT 2
#define MPJX_MPJBUF_OVERRUN 3
#define MPJX_MPJBUF_TOO_MANY_SECTIONS 4
int mpjx_mpjbuf_combine(int op, int type, void *acc, const void *msg, int64_t msg_bytes, int64_t count,
                        int *status, unsigned flags, void *stream);

/* ---- communicators ----------------------------------------------------------------------------- */
/* One process per GPU over RCCL (the niodev/native-device deployment): rank 0 creates the id,
 * every rank calls mpjx_comm_init_rank with it. Replaces MPJDev.init + the COMM_WORLD Intracomm
 * (src/mpi/MPI.java:298-305). Blocking waits on such a communicator poll RCCL's asynchronous error
 * state; an error, or a call still incomplete after MPJX_RCCL_TIMEOUT_S seconds (unset: no limit),
 * aborts the communicator (ncclCommAbort) and returns MPJX_ERR_RCCL, and every later call on it fails
 * the same way, instead of the rank hanging on a dead peer. The routing knobs MPJX_RCCL_P2P (grouped
 * send/recv exchanges) and MPJX_RCCL_NATIVE / MPJX_RCCL_NATIVE_P2 (one ncclAllReduce where the result is
 * order-free) are read HERE, once per communicator, and checked equal on every rank (collective; ranks
 * that differ all get MPJX_ERR_ARG); later changes to the environment do not affect the communicator. */
int mpjx_get_unique_id(mpjx_unique_id *id);
int mpjx_comm_init_rank(mpjx_comm_t *comm, int nranks, const mpjx_unique_id *id, int rank, int device);
/* Multicore mode: nranks ranks that are threads of THIS process (smpdev,
 * src/runtime/starter/MulticoreStarter.java:309-322), rank r on devices[r] (devices may repeat).
 * Fills comms[0..nranks). Each rank's thread then drives its own comm. When every device pair has
 * peer access, the collectives read and write the other ranks' buffers directly (one kernel, two
 * host rendezvous; all ranks on one device: rank 0 launches for everyone), so every rank's buffers
 * must stay valid until all ranks' calls have returned and their streams passed the call.
 * MPJX_SMP_COPY=1 selects copy-based exchanges instead. */
int mpjx_comm_init_smp(mpjx_comm_t *comms, int nranks, const int *devices);
/* The same multicore world formed by the rank threads one by one (smpdev: every rank thread runs
 * MPI.Init and creates each communicator itself, MulticoreStarter.java:309-322; NativeIntracomm's
 * Split/Create, src/mpi/NativeIntracomm.java:160-215): every rank thread of a world calls it with
 * the world's id (any 128 bytes unique to it, shared over the host Bcast) and all ranks' devices.
 * The first caller creates every handle; each caller gets its own. Non-blocking. Every caller must
 * pass the same nranks and devices[] (a mismatch is MPJX_ERR_ARG). The registry keeps a world until
 * its last rank has taken its handle: a rank thread that never arrives leaves the others' handles
 * usable only for calls that do not need it (a collective would wait for it). */
int mpjx_comm_init_smp_rank(mpjx_comm_t *comm, int nranks, const mpjx_unique_id *id, int rank,
                            const int *devices);
/* Processes of one node without RCCL (several niodev/native-device ranks on one host, one per GPU or
 * several sharing a GPU): each rank maps the other ranks' device buffers through HIP IPC and every
 * collective runs on the direct engine above (one P-way kernel per rank reading every rank's send
 * block and writing every rank's recv block over xGMI, between two host barriers). `id` is any 128
 * bytes unique to this world, shared out of band (mpjx_get_unique_id works); the ranks rendezvous
 * through a POSIX shared-memory segment named from it, so they must share /dev/shm. Buffers must
 * be hipMalloc'd device memory (any offset into an allocation). A rank that fails or does not
 * arrive within MPJX_IPC_TIMEOUT_S seconds (default 300) makes every rank's call fail instead of
 * hanging. MPJX_SMP_COPY=1 selects copy-based exchanges (pulls from the mapped buffers). */
int mpjx_comm_init_ipc(mpjx_comm_t *comm, int nranks, const mpjx_unique_id *id, int rank, int device);
int mpjx_comm_destroy(mpjx_comm_t comm);
int mpjx_comm_rank(mpjx_comm_t comm, int *rank);
int mpjx_comm_size(mpjx_comm_t comm, int *size);
int mpjx_comm_device(mpjx_comm_t comm, int *device);
int mpjx_comm_stream(mpjx_comm_t comm, void **stream);
int mpjx_comm_synchronize(mpjx_comm_t comm);
int mpjx_barrier(mpjx_comm_t comm);

/* ---- collectives on device-resident buffers (IntracommImpl, src/mpi/IntracommImpl.java:426-503) ---- */
/* Intracomm.Reduce (src/mpi/Intracomm.java:740-760 -> PureIntracomm.java:1923-1992): result on
 * `root`. Default order = MST_Reduce tree. Without MPJX_FLAG_FAITHFUL the recvbuf of other ranks is
 * neither read nor written (may be NULL there). With MPJX_FLAG_FAITHFUL recvbuf is significant and
 * WRITTEN on every rank: its MST sub-tree partial (default), or a copy of its own sendbuf (with
 * MPJX_FLAG_OLD_COLLECTIVES) — see MPJX_FLAG_FAITHFUL. */
int mpjx_reduce(mpjx_comm_t comm, const void *sendbuf, void *recvbuf, int64_t count, int type, int op,
                int root, unsigned flags, void *stream);
/* Intracomm.Allreduce (src/mpi/Intracomm.java:787-793 -> PureIntracomm.java:2168-2185): default
 * order = MST_Reduce(root 0) + MST_Bcast, identical bits on every rank. In-place allowed. */
int mpjx_allreduce(mpjx_comm_t comm, const void *sendbuf, void *recvbuf, int64_t count, int type,
                   int op, unsigned flags, void *stream);
/* Intracomm.Reduce_scatter (src/mpi/Intracomm.java:833-840 -> PureIntracomm.java:2355-2456):
 * rank r receives recvcounts[r] elements (block r of the reduced vector). sendbuf is read only,
 * except with MPJX_FLAG_FAITHFUL (default order, P >= 2, non-pair types), where the call ends by
 * overwriting the caller's sendbuf as the reference's bucket ring does — see MPJX_FLAG_FAITHFUL. */
int mpjx_reduce_scatter(mpjx_comm_t comm, const void *sendbuf, void *recvbuf, const int64_t *recvcounts,
                        int type, int op, unsigned flags, void *stream);
/* Intracomm.Scan (src/mpi/Intracomm.java:879-885 -> PureIntracomm.java:2495-2545): inclusive
 * prefix, rank r gets x_{r-1} (op) (... (op) (x_0 (op) x_r)) — the reference's fold order. */
int mpjx_scan(mpjx_comm_t comm, const void *sendbuf, void *recvbuf, int64_t count, int type, int op,
              unsigned flags, void *stream);
/* Measurement: with enable != 0, mpjx_allreduce, mpjx_reduce_scatter and mpjx_scan record HIP timing
 * events at their phase boundaries on the call's stream (one communicator, cheap, off by default).
 * mpjx_comm_last_phases waits for the last instrumented call and returns its three phase durations in
 * ms and the engine that ran it:
 *   *engine = 1  exchange engine (RCCL, or copy exchanges): exchange #1 / P-way combine / exchange #2
 *                (Reduce_scatter has no exchange #2: ms3[2] ~ 0, or the faithful sendbuf rewrite)
 *   *engine = 2  direct engine (multicore, HIP-IPC): share (incl. IPC pushes + rendezvous) / combine /
 *                fence (incl. IPC copy-out + rendezvous)
 *   *engine = 3  chunk-pipelined Allreduce: ms3[0] = the whole call (its phases overlap), others -1
 *   *engine = 4  one-rank communicator: ms3[1] = the copy send -> recv (ms3[0], ms3[2] ~ 0)
 *   *engine = 5  one-shot (small vectors): all-gather of the whole vectors / combine / - (~0)
 *   *engine = 6  one ncclAllReduce (MPJX_RCCL_NATIVE=1 where the result is order-free): ms3[1]
 * A windowed call (the IPC engine over vectors longer than its staging region) reports its last window.
 * An instrumented call that took a path without phase marks (Reduce, Bcast, ...) makes the next
 * mpjx_comm_last_phases fail with MPJX_ERR_ARG rather than return an earlier call's phases.
 * No reference counterpart (bench.py's N > 1 "phases" breakdown). */
int mpjx_comm_phase_timing(mpjx_comm_t comm, int enable);
int mpjx_comm_last_phases(mpjx_comm_t comm, float *ms3, int *engine);
/* For an instrumented chunk-pipelined Allreduce (*engine = 3): per chunk k, six times in ms from the
 * call's start — exchange #1 start/end (call stream), combine start/end (combine stream), all-gather
 * start/end (gather stream, the transport's second lane) — into ms[6k .. 6k+5], for at most cap / 6
 * chunks; *nchunks = the chunks written. Shows which intervals overlapped. */
int mpjx_comm_pipeline_trace(mpjx_comm_t comm, float *ms, int cap, int *nchunks);
/* Intracomm.Bcast (PureIntracomm.java:592-736), phase 2 of the reference Allreduce. */
int mpjx_bcast(mpjx_comm_t comm, void *buf, int64_t count, int type, int root, void *stream);
/* Intracomm.Gather (PureIntracomm.java:782-1053, MST/FT): `count` elements from every rank land at
 * recvbuf + r*count on the root (recvbuf significant at the root only). */
int mpjx_gather(mpjx_comm_t comm, const void *sendbuf, void *recvbuf, int64_t count, int type, int root,
                void *stream);
/* Intracomm.Scatter (PureIntracomm.java:1055-1171): rank r receives the root's sendbuf + r*count
 * (sendbuf significant at the root only); root delivery step of FT_Reduce_scatter (:2454). */
int mpjx_scatter(mpjx_comm_t comm, const void *sendbuf, void *recvbuf, int64_t count, int type, int root,
                 void *stream);

/* ---- block moves (Intracomm.Allgather .. Alltoallv, src/mpi/Intracomm.java:363-690) -----------------
 * Device pointers; counts and displacements in ELEMENTS of `type` (a pair type's element is one pair),
 * displacements from the start of the buffer they index, in any order, with gaps. The data is moved as
 * plain bytes, so the calls take no flags and no byte order applies. Enqueued on `stream` and ordered
 * like every other call. The buffers may sit at any byte alignment.
 *   MPJX_ERR_ARG: a negative count or displacement, a NULL buffer or table with a nonzero count, an
 *   unknown type, a bad root, a buffer that is not GPU-accessible, two receive segments of this rank
 *   that overlap, or this rank's send and receive ranges overlapping (mpiJava has no in-place form).
 * Count tables are significant where MPI says: recvcounts/displs of mpjx_gatherv and sendcounts/displs of
 * mpjx_scatterv at the root only (as are recvbuf and sendbuf there).
 * One rank, and multicore ranks sharing one device (MPJX_SMP_COPY unset): one launch of the block-move
 * kernel for the whole world; there every rank sees every table, and a send count that differs from the
 * matching receive count is MPJX_ERR_ARG on every rank before anything moves. In every other world
 * (RCCL, HIP-IPC, multicore across devices, MPJX_SMP_COPY=1) the rank's own block is moved by that
 * kernel and the rest by the transport's exchanges, and matching counts between ranks are the caller's
 * contract, as in MPI. */
/* Intracomm.Allgather: every rank's `count` elements land at recvbuf + r*count on every rank. */
int mpjx_allgather(mpjx_comm_t comm, const void *sendbuf, void *recvbuf, int64_t count, int type,
                   void *stream);
/* Intracomm.Allgatherv: rank r's sendcount (= every rank's recvcounts[r]) elements land at
 * recvbuf + displs[r] on every rank. */
int mpjx_allgatherv(mpjx_comm_t comm, const void *sendbuf, int64_t sendcount, void *recvbuf,
                    const int64_t *recvcounts, const int64_t *displs, int type, void *stream);
/* Intracomm.Gatherv: rank r's sendcount elements land at recvbuf + displs[r] on the root. */
int mpjx_gatherv(mpjx_comm_t comm, const void *sendbuf, int64_t sendcount, void *recvbuf,
                 const int64_t *recvcounts, const int64_t *displs, int type, int root, void *stream);
/* Intracomm.Scatterv: rank r receives sendcounts[r] (= its recvcount) elements from the root's
 * sendbuf + displs[r]. */
int mpjx_scatterv(mpjx_comm_t comm, const void *sendbuf, const int64_t *sendcounts, const int64_t *displs,
                  void *recvbuf, int64_t recvcount, int type, int root, void *stream);
/* Intracomm.Alltoall: block j (count elements at sendbuf + j*count) goes to rank j, which stores the
 * block from rank i at recvbuf + i*count. */
int mpjx_alltoall(mpjx_comm_t comm, const void *sendbuf, void *recvbuf, int64_t count, int type,
                  void *stream);
/* Intracomm.Alltoallv: sendcounts[j] elements at sendbuf + sdispls[j] go to rank j; recvcounts[i]
 * elements from rank i land at recvbuf + rdispls[i]. */
int mpjx_alltoallv(mpjx_comm_t comm, const void *sendbuf, const int64_t *sendcounts, const int64_t *sdispls,
                   void *recvbuf, const int64_t *recvcounts, const int64_t *rdispls, int type, void *stream);

/* ---- derived datatypes and the strided block move (src/mpi/Contiguous.java, src/mpi/Vector.java) -------
 * A derived type normalises to `nblocks` blocks of `blocklen` elements of its basic type, `stride` elements
 * apart: size = nblocks*blocklen, extent = (nblocks-1)*stride + blocklen (0 for an empty type, as
 * Vector.computeBounds gives for a positive stride), lb = 0. `oldtype` is a basic code, a pair code (which is
 * Contiguous(2, base)) or a derived code that is itself contiguous; stride is in units of oldtype's extent.
 * Vector(c, b, b, T), count <= 1 and an empty block normalise to contiguous.
 *   MPJX_ERR_ARG: a negative count or blocklength, an unknown or freed oldtype, sizes beyond 2^62 bytes.
 *   MPJX_ERR_UNSUPPORTED (the message names what was passed): a stride smaller than the block length
 *   (negative, zero or overlapping), a strided oldtype (Vector of Vector, Contiguous of Vector).
 * An oldtype with explicit bounds (made by mpjx_type_struct with a marker, below) is accepted by both: its items
 * lie one explicit extent apart, the bounds follow Contiguous.java:71-98 (extent = count*old.extent, lb = old.lb,
 * ub = lb + extent) and Vector.java:99-135, the sticky flags are handed on, and the blocks are flattened through
 * the planner of the irregular types below; the result is regular again where its blocks are.
 * Derived codes are handles >= 0x10000 from a process-wide, thread-safe registry, local to the rank as MPI
 * types are (only the signatures must match between ranks). A freed code is never reissued; a freed or
 * unknown code is MPJX_ERR_ARG in every later call. mpjx_type_size() returns 0 for a derived code, so every
 * entry point above rejects one as an unknown datatype; mpjx_type_info is the authority for them (and
 * answers basic and pair codes too: base = the basic code, size and extent in its elements). */
int mpjx_type_contiguous(int64_t count, int oldtype, int *newtype);
int mpjx_type_vector(int64_t count, int64_t blocklength, int64_t stride, int oldtype, int *newtype);
int mpjx_type_free(int type);
int mpjx_type_info(int type, int *base, int64_t *size, int64_t *extent);
/* ---- irregular datatypes (src/mpi/Hvector.java, src/mpi/Indexed.java, src/mpi/Hindexed.java) ------------
 * A list of blocks (offset, length) in elements of the basic type from the item's origin, kept in PACK order:
 * the order of the constructor's arrays, not address order.
 *   Indexed(bl[], disp[], old)   block i is bl[i] items of old, old.extent apart, starting disp[i]*old.extent
 *                                elements from the origin
 *   Hindexed                     the same, but block i starts at disp[i] elements: mpiJava's "H" units are
 *                                buffer indices, not bytes
 *   Hvector(count, bl, stride, old)   block j starts j*stride elements from the origin
 * size = sum bl*old.size; lb = the minimum over non-empty blocks of start + old.lb; ub = the maximum of
 * start + (bl-1)*old.extent + old.ub; extent = ub - lb; an empty type has all four 0. Zero-length blocks take
 * no part in the bounds. Item k of a message starts k*extent after item 0's origin and block offsets are added
 * to that origin: lb is NOT subtracted, so Indexed([2],[3],INT) has lb 3 and extent 2 and its item k is elements
 * 3+2k, 4+2k past the buffer position.
 * oldtype is any live type: basic, pair, Contiguous, Vector or one of these. A non-contiguous oldtype is
 * flattened into the list; consecutive blocks that abut in pack order and in address order are merged. A list
 * that is regular (equal lengths at a constant positive stride of at least the length, in order, first offset
 * 0) IS the Vector of that shape and takes its path. mpjx_type_vector and mpjx_type_contiguous still reject
 * every non-contiguous oldtype: Hvector(c, b, s*old.extent, old) is the supported spelling of a Vector of a
 * Vector.
 * A type whose own blocks share a byte is legal to send; as a receive type it is MPJX_ERR_ARG.
 *   MPJX_ERR_ARG: a negative block length or count, n < 0, NULL arrays with n > 0, an unknown or freed
 *   oldtype, sizes beyond 2^62 bytes.
 *   MPJX_ERR_UNSUPPORTED (the message names what was passed): a negative displacement (lb < 0), an Hvector
 *   stride < 1 with count > 1, more than 1,048,576 blocks after merging (a type's device table is 16 B per
 *   block).
 * mpjx_type_layout: lb and ub in elements of the basic type (0 and the extent for every regular type without
 * explicit bounds; the explicit ones for a type made with the markers of mpjx_type_struct, below), the
 * merged block count, and regular = 1 if the type takes the block-move or strided kernel, 0 if the indexed
 * one. mpjx_type_info, mpjx_type_free and mpjx_alltoallv_dt take the new codes like the others; a call
 * enqueued before mpjx_type_free completes with the layout it was given. */
int mpjx_type_hvector(int64_t count, int64_t blocklength, int64_t stride, int oldtype, int *newtype);
int mpjx_type_indexed(int n, const int64_t *blocklengths, const int64_t *displacements, int oldtype, int *newtype);
int mpjx_type_hindexed(int n, const int64_t *blocklengths, const int64_t *displacements, int oldtype, int *newtype);
int mpjx_type_layout(int type, int64_t *lb, int64_t *ub, int64_t *nblocks, int *regular);
/* ---- Struct and the LB / UB markers (src/mpi/Struct.java) --------------------------------------------------
 * Struct(bl[], disp[], types[]): block i is bl[i] items of types[i], one extent of that type apart, starting
 * disp[i] elements of the BASIC type from the origin; the blocks are packed in the order of the arrays
 * (StructPacker.pack, Struct.java:448-464). types[i] is any live type or a marker, MPJX_LB / MPJX_UB. All
 * components that are not markers must have one basic type, which makes a Struct one mpjbuf section like every
 * other type. The blocks are flattened, merged, stripped of empty ones and normalised as for Indexed: a Struct
 * whose data blocks are regular IS the Vector of that shape (regular = 1) and takes its path.
 * Bounds: Struct.computeBounds (Struct.java:149-386) AS WRITTEN, in the order of the arrays, which is NOT
 * MPI's "markers are sticky minima and maxima":
 *   - a component with ubSet (an UB marker, or a type made from one) REPLACES ub with
 *     disp + (bl-1)*extent + its ub: the `if (max_ub > ub)` test is commented out (Struct.java:242-244), so a
 *     later marker replaces an earlier one, higher or lower;
 *   - a component without ubSet moves ub to max(its end, disp) whenever its end reaches past every earlier
 *     such component's (trueUb, Struct.java:251-258), even after a marker: a data block after a marker can
 *     move ub again;
 *   - lb mirrors both rules (Struct.java:272-303);
 *   - a marker is itself a component without the flag for the OTHER bound (an LB at 10 before any data sets ub
 *     to 10), and components of length 0 take no part.
 * extent = ub - lb; lbSet / ubSet are sticky: every constructor hands them on with the bounds its own class
 * computes (Contiguous, Vector, Hvector, Indexed, Hindexed: the minimum and maximum over the blocks of
 * start + old.lb and start + (bl-1)*old.extent + old.ub). mpiJava 1.2 has no Type_create_resized: a Struct with
 * an UB marker is how a type is resized, e.g. a column of a row-major matrix to an extent of one element, so
 * that `count` items are `count` adjacent columns.
 * Item k of a message starts k*extent after the origin and lb is NOT subtracted (GenericPacker). Extent 0 with
 * data is legal: every item lies at the same place, which can be sent; receiving more than one such item is
 * MPJX_ERR_ARG by the self-overlap rule. The blocks of an item may reach past the next item's origin; whether
 * two items of a receive layout share a byte is part of the exact overlap check of mpjx_alltoallv_dt.
 * mpjx_type_info and mpjx_type_layout report these bounds (extent = ub - lb); the layout a call touches is
 * always the blocks' own.
 *   MPJX_ERR_ARG: n < 0, NULL arrays with n > 0, a negative block length, an unknown or freed component type,
 *   components of different basic types ("Base types of all component types in a Struct must agree"), sizes
 *   beyond 2^62 bytes.
 *   MPJX_ERR_UNSUPPORTED (the message names the value): DATA at a negative displacement (a marker at one is
 *   fine: lb < 0), an explicit extent below 0 (ub < lb), more than 1,048,576 blocks after merging. */
int mpjx_type_struct(int n, const int64_t *blocklengths, const int64_t *displacements, const int *types,
                     int *newtype);
/* The blocks' own bounds, in elements of the basic type from the item's origin: the lowest element an item
 * touches and one past the highest (both 0 for an empty type). They equal lb and ub unless the type carries
 * explicit bounds; `count` items touch [true_lb, (count-1)*extent + true_ub), which is what a buffer must hold.
 *   MPJX_ERR_ARG: an unknown or freed type, a marker. */
int mpjx_type_true_bounds(int type, int64_t *true_lb, int64_t *true_ub);
/* The general block move: sendcounts[j] items of sendtype, the first at sendbuf + sdispls[j], go to rank j;
 * recvcounts[i] items of recvtype from rank i land from recvbuf + rdispls[i]. Every block move and every
 * rooted call is a special case, with zero counts where a rank has nothing to send or receive.
 * Counts are ITEMS of the side's type; item k of a message lies k extents after the first. Displacements are
 * in elements of the BASIC type, as the reference's v-calls add them to the buffer offset
 * (PureIntracomm.java:984,1232,1630,1832,1848): Alltoallv with a Vector send type is a transpose without a
 * resized type. A message's packed form is its blocks in order; a send matches a receive when both types have
 * the same basic type and the packed lengths are equal, and the packed bytes are stored in order into the
 * receive layout (the block shapes need not agree). Only bytes inside receive blocks are written.
 *   MPJX_ERR_ARG: as for the block moves above, an unknown or freed type, types of different basic types,
 *   two receive layouts of this rank that share a byte, or a send layout that shares a byte with a receive
 *   layout. That check is exact (two interleaved columns of one matrix do not overlap): layouts whose
 *   bounding spans are disjoint are settled at any size; where spans meet, the blocks are compared while the
 *   call's tables hold at most 65,536 blocks in total; beyond that it is skipped and disjoint layouts are
 *   the caller's contract, as in MPI.
 *   MPJX_ERR_UNSUPPORTED: one message of 2^32 or more granules (the largest power of two <= 16 B that divides
 *   both layouts' block bytes, strides, extents and addresses; for an irregular type, every block offset and length).
 * No flags and no faithful mode. Enqueued on `stream`, ordered and failure-marked like the other collectives.
 * A segment whose two layouts are contiguous runs the block-move kernel, one whose two layouts are regular the
 * strided kernel — or, where one layout is a contiguous run and the other has one granule (1, 2, 4, 8 or 16
 * bytes) per block, consecutive items on consecutive granules, two or more blocks and two or more items (the
 * element transpose: columns resized to one element), the transpose kernel, which moves tiles through LDS so
 * that both sides are read and written in consecutive granules; MPJX_TRANSPOSE=0 in the environment, read per
 * call, keeps the strided kernel for these — every other one the indexed kernel (a binary search of the type's block table per granule; the
 * table is uploaded once per communicator and type, on the stream of the first call that uses it).
 * One rank, and multicore ranks sharing one device (MPJX_SMP_COPY unset): one launch per kernel for the whole
 * world; a base-type or packed-length mismatch between a sender and its receiver is MPJX_ERR_ARG on every
 * rank before anything moves. In every other world the rank's own block moves from layout to layout, strided
 * sends are packed into communicator scratch, the packed bytes go through the transport's exchange and
 * strided receives are unpacked; a contiguous side is sent from, or received into, its buffer, and matching
 * signatures are the caller's contract. */
int mpjx_alltoallv_dt(mpjx_comm_t comm,
                      const void *sendbuf, const int64_t *sendcounts, const int64_t *sdispls, int sendtype,
                      void *recvbuf, const int64_t *recvcounts, const int64_t *rdispls, int recvtype,
                      void *stream);

/* ---- reductions on derived datatypes ------------------------------------------------------------------
 * mpjx_reduce / _allreduce / _reduce_scatter / _scan with `type` a basic, pair OR derived code; the other
 * arguments are their counterparts'. With a basic or pair code each call IS its counterpart.
 * With a derived code, `count` items of `type` are read from sendbuf and written to recvbuf: item k starts
 * k * extent after the buffer position and lb is not subtracted, as in mpjx_alltoallv_dt. The reduction is
 * element-wise over the PACKED sequence of base elements — over (value, index) pairs for a type made of a pair
 * type, which is what MPJX_MAXLOC / MPJX_MINLOC take — in the combine order of the counterpart on the packed
 * vectors (the MST tree rooted at `root`, at 0 for Allreduce; FT under MPJX_FLAG_OLD_COLLECTIVES; the Scan
 * fold; Reduce_scatter's rule by P), so the results are bit-identical to it. Only bytes inside the type's
 * blocks are written: gaps of recvbuf keep their contents. Reduce: recvbuf is significant at the root only
 * and may be NULL elsewhere. Reduce_scatter: recvcounts are in items, sendbuf holds their sum, and rank r's
 * recvcounts[r] items are laid out from recvbuf's own origin. The (op, type) pair is valid exactly when
 * mpjx_op_check(op, the base or pair type) accepts it. In one call, either every rank passes a basic or pair
 * code or every rank a derived one. The reference defines no result here (PureIntracomm.Reduce copies
 * count * size contiguous elements whatever the type): these calls follow MPI.
 *   MPJX_ERR_ARG: an unknown or freed type; a type whose own blocks share a byte; on one rank, a send layout
 *   that shares a byte with its receive layout, other than exactly in place (sendbuf == recvbuf;
 *   Reduce_scatter, whose two layouts differ, has no in-place form) — the exact check and the 65,536-block
 *   limit of mpjx_alltoallv_dt; where every rank sees every rank's call (multicore ranks on one device,
 *   2 <= P <= 8), ranks whose base type or packed length differ: there these errors, and a rank's overlap, are
 *   returned on every rank before anything moves.
 *   MPJX_ERR_OP_TYPE: as mpjx_op_check, on the base type.
 *   MPJX_ERR_UNSUPPORTED: MPJX_FLAG_FAITHFUL, MPJX_FLAG_SEND_BIG_ENDIAN or MPJX_FLAG_RECV_BIG_ENDIAN with a
 *   derived type; 2^32 or more granules in one call.
 * Asynchronous on `stream`; MPJX_FLAG_BLOCKING is honoured; a failing rank fails its world like every
 * collective; mpjx_type_free between enqueue and completion changes nothing.
 * Forms (mpjx_comm_last_dt_form, the last *_dt call of this rank; no reference counterpart, tests read it):
 *   MPJX_DT_FORM_CONTIGUOUS  a basic or pair code: the contiguous call
 *   MPJX_DT_FORM_MOVE        one rank: the copy of send into recv through the layouts; in place, nothing
 *   MPJX_DT_FORM_DIRECT      multicore ranks on one device, 2 <= P <= 8, MPJX_SMP_COPY unset, every rank's
 *                            type of one normal form: one layout-aware P-way combine kernel launched by rank
 *                            0 reads every rank's send layout and writes every receive layout in one pass
 *   MPJX_DT_FORM_PACK        every other world, and ranks whose types differ in form: sendbuf packed into a
 *                            staging region of the communicator, the contiguous call on the packed vectors,
 *                            the result unpacked into recvbuf (a contiguous layout skips both passes) */
#define MPJX_DT_FORM_CONTIGUOUS 1
#define MPJX_DT_FORM_MOVE 2
#define MPJX_DT_FORM_DIRECT 3
#define MPJX_DT_FORM_PACK 4
int mpjx_reduce_dt(mpjx_comm_t comm, const void *sendbuf, void *recvbuf, int64_t count, int type, int op,
                   int root, unsigned flags, void *stream);
int mpjx_allreduce_dt(mpjx_comm_t comm, const void *sendbuf, void *recvbuf, int64_t count, int type,
                      int op, unsigned flags, void *stream);
int mpjx_reduce_scatter_dt(mpjx_comm_t comm, const void *sendbuf, void *recvbuf, const int64_t *recvcounts,
                           int type, int op, unsigned flags, void *stream);
int mpjx_scan_dt(mpjx_comm_t comm, const void *sendbuf, void *recvbuf, int64_t count, int type, int op,
                 unsigned flags, void *stream);
int mpjx_comm_last_dt_form(mpjx_comm_t comm, int *form);
/* The kernels this rank's last data-movement call launched (the nine block moves; the P = 1 and pack forms of
 * the *_dt reductions set it too), one bit each; 0 on a rank that launched nothing — in a multicore world on
 * one device rank 0 launches for the world. No reference counterpart, tests read it.
 *   MPJX_ERR_ARG: comm or mask is NULL. */
#define MPJX_MOVE_KERNEL_MOVES 1u
#define MPJX_MOVE_KERNEL_STRIDED 2u
#define MPJX_MOVE_KERNEL_INDEXED 4u
#define MPJX_MOVE_KERNEL_TRANSPOSE 8u
int mpjx_comm_last_move_kernels(mpjx_comm_t comm, unsigned *mask);

/* ---- Pack, Unpack, Pack_size (Comm.Pack / Unpack / Pack_size, src/mpi/Comm.java:1860-1983) ----------------
 * `count` items of any datatype (basic, pair or derived) to and from ONE section of an mpjbuf static-buffer
 * image, the form mpjx_mpjbuf_combine, niodev and the Java side read. A section starts at
 * h = round_up(position, 8) (src/mpjbuf/Buffer.java:609-704, NIOBuffer.java:520-563):
 *   byte h          the mpjbuf type code = the base type's code - 1
 *   bytes h+1..h+3  zero
 *   bytes h+4..h+7  big-endian int32 count of BASE elements (count * the type's size; a pair is 2)
 *   from h+8        the elements in PACK order (item by item, blocks in the constructor's order), each base
 *                   word big-endian; a pair type's words are its base type's
 * *position goes in and comes out as h + 8 + the payload's bytes; it is computed on the host. The reference
 * writes the count field only at the next putSectionHeader or at commit(); mpjx_pack writes it at once, so
 * the image after the call is the committed one. Bytes between position and h are left as they were.
 * count == 0 writes (or expects) a header with count 0.
 * One kernel does layout, byte swap and header in a single pass (k_pack). Both calls are LOCAL, not
 * collective: they take the communicator for its stream convention (enqueued on `stream`, ordered after its
 * previous call, asynchronous like the *_dt calls) and for its cache of the irregular types' device tables.
 * inbuf / outbuf is the buffer position of item 0; item k lies k extents on and lb is NOT subtracted, as in
 * mpjx_alltoallv_dt. image is device memory or pinned host memory (mpjx_host_alloc); it must not share bytes
 * with the buffer.
 *   MPJX_ERR_ARG, before anything is launched: an unknown or freed type; a NULL position, image or (unpack)
 *   status; a NULL inbuf / outbuf with a nonzero count; a negative count or position; count * size above
 *   2^31 - 1 (the header field is a Java int); inbuf / outbuf not aligned to the base element (a Java array
 *   always is); image not 8-byte aligned; a section that would end past image_bytes (mpjx_pack checks what it
 *   really needs, not mpjx_pack_size); for mpjx_unpack a type whose own blocks share a byte; memory that is
 *   not GPU-accessible. These are checked before the communicator is looked at.
 * mpjx_unpack reads exactly one section at round_up(*position, 8) into `count` items. The kernel reads the
 * header itself (the image may have arrived in device memory) before any payload byte: a wrong type code
 * (MPJX_MPJBUF_BAD_TYPE), a count whose payload passes image_bytes (MPJX_MPJBUF_OVERRUN) or a count that is
 * not count * size (MPJX_MPJBUF_BAD_COUNT) leave outbuf untouched and store that code into *status, a
 * device-accessible int the caller zeroes (the contract of mpjx_mpjbuf_combine); *position still advances by
 * the expected section. Bytes of outbuf between the type's blocks keep their contents.
 * mpjx_pack_size returns the reference's value, padding quirk included: t = 8 + count * size in bytes,
 * *bytes = t + t % 8 (src/mpi/BasicType.java:209-220). It is an upper bound of what mpjx_pack writes only for
 * a section that starts at a multiple of 8: from position 1, INT x 2 occupies bytes 8..23 of the image, while
 * 1 + mpjx_pack_size = 17. */
int mpjx_pack_size(int64_t count, int type, int64_t *bytes);
int mpjx_pack(mpjx_comm_t comm, const void *inbuf, int64_t count, int type, void *image, int64_t image_bytes,
              int64_t *position, void *stream);
int mpjx_unpack(mpjx_comm_t comm, const void *image, int64_t image_bytes, int64_t *position, void *outbuf,
                int64_t count, int type, int *status, void *stream);

/* ---- point-to-point: Send, Recv, Isend, Irecv, Sendrecv, Sendrecv_replace, Wait, Test, Waitall -------------------
 * (src/mpi/Comm.java:381, :882, :1446, :1578, :2301, :2392; src/mpi/Request.java:81, :159; src/mpi/Status.java)
 * One message from one rank to another, on device buffers, with any datatype on either side (the packed bytes
 * of the send layout, in order, into the receive layout, as mpjx_alltoallv_dt moves them). count is in items of
 * `type`; buf is the address of the first base element.
 *
 * Matching is MPI's, per world: a send (source, dest, tag) matches the first posted receive at dest, in post
 * order, whose source is the sender or MPJX_ANY_SOURCE and whose tag is the send's or MPJX_ANY_TAG; a receive
 * matches the first unmatched send likewise, so messages of one (source, dest) do not overtake. A send tag
 * is >= 0. A MPJX_PROC_NULL peer completes at once: source MPJX_PROC_NULL, tag MPJX_ANY_TAG, 0 elements.
 * Point-to-point and collective traffic never meet, and a sub-communicator matches apart from its parent.
 *
 * At match time both types must be made of the same basic type and the message's packed bytes must fit the
 * receive layout (recvcount items). A shorter message is legal: the first n packed bytes of the receive layout
 * are written and the rest keeps its contents. A base-type mismatch, an over-long message or a self-message whose
 * two layouts share a byte completes BOTH requests with MPJX_ERR_ARG (mpjx_last_error names both envelopes);
 * nothing is moved and the world stays usable. A receive type whose own blocks share a byte is MPJX_ERR_ARG at
 * post. Argument errors found before posting (a bad rank, a negative count or tag, NULL with a nonzero count, an
 * unknown or freed type) post nothing and do not fail the world.
 *
 * Nothing is launched at post time. A call that waits (mpjx_wait, mpjx_waitall, mpjx_test and the blocking
 * calls) claims EVERY matched, unclaimed message its rank is a party to, sender or receiver, moves the whole
 * batch on the communicator's stream — one k_msgs launch per table_max messages (mpjx_comm_p2p_stats), whatever their
 * layouts; element transposes go to k_transpose — and the other party's wait then orders its stream after that
 * batch. Either party can move a matched message, so no legal order of waits deadlocks. mpjx_wait and
 * mpjx_waitall return once the data is complete on the host's view; mpjx_test never blocks. A wait on an
 * unmatched request sleeps on the host and enqueues nothing on the GPU.
 *
 * Every host wait is bounded: MPJX_P2P_TIMEOUT_S seconds (default 300, read once when the world is created),
 * or mpjx_comm_set_p2p_timeout for this rank. On expiry the call returns MPJX_ERR_INTERNAL naming the
 * unmatched envelope and the world is marked failed: every peer's wait and later call errors out.
 *
 * mpjx_send of at most MPJX_P2P_EAGER_KIB packed KiB (default 128, the reference's protocol switch limit,
 * src/runtime/starter/MPJRun.java:76; read once per world) is eager: the message is packed into a per-rank device
 * slab of MPJX_P2P_EAGER_POOL_MIB MiB (default 8, src/mpjbuf/BufferConstants.java:28) on the rank's stream, posted
 * as a contiguous message of the base type, and the call returns. With no room in the slab, or above the limit,
 * mpjx_send is mpjx_isend + mpjx_wait. mpjx_isend never copies: the buffer is the caller's until the wait, as in
 * MPI (the reference packs at Isend). MPJX_P2P_BATCH=0 (read once per world) moves a batch with one launch per
 * kernel family instead of k_msgs: a comparison switch.
 *
 * Provided for multicore worlds (mpjx_comm_init_smp, _smp_rank) whose ranks address each other's memory, P = 1
 * included; RCCL, IPC and other worlds return MPJX_ERR_UNSUPPORTED. Not provided: Bsend / Ssend / Rsend
 * and their _init forms, Waitany / Waitsome / Test*all, Cancel, host arrays, big-endian and faithful modes,
 * MPI.OBJECT. Persistent requests, MPI.PACKED messages and Probe / Iprobe are provided: see below.
 *
 * mpjx_status.elements is the received base elements (for a receive type of size 0: the receive count);
 * mpjx_get_count follows Comm.java:1517-1531: *count = elements / size if that divides, else MPJX_UNDEFINED; for a
 * type of size 0, *count = status->elements and *elements = MPJX_UNDEFINED. A request handle is set to NULL on
 * completion or free (a persistent one: on free only). mpjx_comm_destroy fails the communicator's pending
 * requests; it does not free under them.
 * mpjx_comm_p2p_stats: for this rank since creation, the k_msgs plus k_transpose launches, the messages it
 * moved, its sends that went eager, and the messages per k_msgs launch. */
enum { MPJX_ANY_SOURCE = -2, MPJX_ANY_TAG = -2, MPJX_PROC_NULL = -3, MPJX_UNDEFINED = -1 }; /* MPI.java:132-136 */
typedef struct mpjx_request *mpjx_request_t;
typedef struct { int source, tag, error; int64_t elements, bytes; } mpjx_status;

int mpjx_isend(mpjx_comm_t comm, const void *buf, int64_t count, int type, int dest, int tag,
               mpjx_request_t *request);
int mpjx_irecv(mpjx_comm_t comm, void *buf, int64_t count, int type, int source, int tag,
               mpjx_request_t *request);
int mpjx_send(mpjx_comm_t comm, const void *buf, int64_t count, int type, int dest, int tag);
int mpjx_recv(mpjx_comm_t comm, void *buf, int64_t count, int type, int source, int tag,
              mpjx_status *status);
int mpjx_sendrecv(mpjx_comm_t comm, const void *sendbuf, int64_t sendcount, int sendtype, int dest,
                  int sendtag, void *recvbuf, int64_t recvcount, int recvtype, int source,
                  int recvtag, mpjx_status *status);
int mpjx_sendrecv_replace(mpjx_comm_t comm, void *buf, int64_t count, int type, int dest,
                          int sendtag, int source, int recvtag, mpjx_status *status);
int mpjx_wait(mpjx_request_t *request, mpjx_status *status);
int mpjx_test(mpjx_request_t *request, int *flag, mpjx_status *status);
int mpjx_waitall(int n, mpjx_request_t *requests, mpjx_status *statuses);
int mpjx_request_free(mpjx_request_t *request);
int mpjx_get_count(const mpjx_status *status, int type, int64_t *count, int64_t *elements);
int mpjx_comm_set_p2p_timeout(mpjx_comm_t comm, double seconds);
int mpjx_comm_p2p_stats(mpjx_comm_t comm, int64_t *launches, int64_t *moved, int64_t *eager,
                        int *table_max);

/* ---- persistent requests: Send_init, Recv_init, Start, Startall ---------------------------------------------------
 * (src/mpi/Comm.java Send_init / Recv_init; src/mpi/Prequest.java:72-119 Start, Startall)
 * mpjx_send_init / mpjx_recv_init run every check mpjx_isend / mpjx_irecv run before posting (type, count, rank,
 * tag, device pointer, a receive layout that shares a byte with itself), once, and return an INACTIVE persistent
 * request: nothing is posted and nothing is enqueued. MPJX_ANY_SOURCE, MPJX_ANY_TAG and MPJX_PROC_NULL are legal
 * where they are for mpjx_irecv and mpjx_isend. A derived type is captured here; freeing it afterwards does not
 * disturb the request. Each persistent request gets a serial number, unique in the process and never reused.
 * A NULL request, a negative count and a negative tag are judged from the arguments alone, before the
 * communicator is looked at (MPJX_ERR_ARG even with a NULL communicator); *request is NULL after any failure.
 *
 * mpjx_start activates the request: to the mailbox it is an mpjx_isend or mpjx_irecv posted now, matched afresh
 * at every start, never eager. mpjx_start on an active request, a request of mpjx_isend / mpjx_irecv or a NULL
 * handle is MPJX_ERR_ARG and posts nothing. mpjx_startall checks every handle first (persistent, inactive, of one
 * communicator, none twice; NULL entries are skipped; on any error nothing is posted), then records at most one
 * ready event for all of them and posts them under one acquisition of the mailbox lock, in array order: the
 * order non-overtaking sees.
 *
 * mpjx_wait, mpjx_test and mpjx_waitall take persistent handles mixed with others. On completion — and on an
 * error of the wait: a mismatch, a timeout — a persistent handle stays non-NULL and becomes inactive; the status
 * of a receive is filled as any receive's. That of a persistent SEND is the empty status (and the error, if
 * any): this differs from a request of mpjx_isend, whose status names the sender and the tag; it is what the
 * reference's programs check ("only the receivers have status values"). A wait or test on an inactive persistent
 * request returns at once with the empty status. mpjx_request_free frees the request and sets the handle to NULL;
 * a pending activation is withdrawn, or, if matched, let go. mpjx_request_is_persistent reports both properties
 * of a handle (0, 0 for NULL).
 *
 * A pair of two persistent requests has the same addresses, layouts and length at every start. The first time a
 * communicator moves such a pair it goes the way of any pair, and its segment is then stored in a slot of a device
 * pool the communicator owns (1024 slots, allocated at first use). A later batch ALL of whose pairs are in the
 * pool goes out in one launch of k_msgs_pool per batch_max (512) pairs, its argument an index of slots instead of
 * a table of table_max segments. Any other batch — one plain pair among them, an element transpose, a pair
 * not stored because the pool is full — takes the path above, unchanged. Slots of freed requests are reused.
 * Storing a segment happens after its batch is enqueued and never fails the exchange: without memory for the
 * pool, or if the store cannot be launched, the pair stays unpooled.
 * MPJX_P2P_POOL=0 (read once per world) keeps every batch on that path: a comparison switch; so does
 * MPJX_P2P_BATCH=0. mpjx_comm_p2p_pool_stats: for this rank since creation, the k_msgs_pool launches (counted in
 * mpjx_comm_p2p_stats' launches too), the segments stored, the pairs moved from the pool, the slots in use now,
 * and the pairs per launch. The three counters are atomic and may be read from any thread, also while the rank's
 * own thread is inside a wait; slots_in_use may be asked for by the rank's own thread only. */
int mpjx_send_init(mpjx_comm_t comm, const void *buf, int64_t count, int type, int dest, int tag,
                   mpjx_request_t *request);
int mpjx_recv_init(mpjx_comm_t comm, void *buf, int64_t count, int type, int source, int tag,
                   mpjx_request_t *request);
int mpjx_start(mpjx_request_t *request);
int mpjx_startall(int n, mpjx_request_t *requests);
int mpjx_request_is_persistent(mpjx_request_t request, int *persistent, int *active);
int mpjx_comm_p2p_pool_stats(mpjx_comm_t comm, int64_t *pool_launches, int64_t *puts, int64_t *hits,
                             int64_t *slots_in_use, int *batch_max);

/* ---- wire-format messages: MPI.PACKED, Probe, Iprobe ------------------------------------------------------------
 * (src/mpi/Comm.java:391-437 send, :1446-1499 recv, :1761 Probe, :1811 Iprobe)
 * In the reference every message is an mpjbuf image: a typed send packs one section and sends the image, a typed
 * receive reads the first section's header and unpacks that many elements, and with MPI.PACKED either side hands
 * over the image itself. MPJX_PACKED is accepted by mpjx_isend, mpjx_irecv, mpjx_send, mpjx_recv, mpjx_sendrecv,
 * mpjx_sendrecv_replace, mpjx_send_init and mpjx_recv_init, and nowhere else. buf is then an mpjbuf image in device
 * memory (the format: "Pack, Unpack, Pack_size" above) and count its length in BYTES: for a send the position
 * mpjx_pack returned, for a receive the room. The image must be 8-byte aligned (MPJX_ERR_ARG at post, nothing is
 * posted). The base-type test at match time passes when either side is PACKED:
 *   PACKED -> PACKED   the image bytes move as a contiguous message; longer than the room is MPJX_ERR_ARG; 0 bytes is
 *                      an empty message.
 *   typed -> PACKED    the receiver's image gets ONE section at position 0: the 8 header bytes, then the send layout's
 *                      elements in pack order, each base word big-endian: byte for byte what mpjx_pack(position 0)
 *                      writes. 8 + payload above the room, or more than 2^31 - 1 base elements, completes both
 *                      requests with MPJX_ERR_ARG at match and moves nothing. 0 items still write a header that
 *                      announces 0. Bytes of the image past the section keep their contents.
 *   PACKED -> typed    the first section of the sent image goes into the receive layout; later sections are ignored
 *                      (the reference reads one header). An image of fewer than 8 bytes is MPJX_ERR_ARG at match. The
 *                      KERNEL reads the header, since the image may have been written by a kernel a moment ago, and
 *                      checks it before it loads any payload byte: a type code other than the receive base type's
 *                      (MPJX_MPJBUF_BAD_TYPE), a negative count n or 8 + n * word bytes above the bytes sent
 *                      (MPJX_MPJBUF_OVERRUN), n above the receive layout's base elements (MPJX_MPJBUF_BAD_COUNT). A
 *                      bad header stores nothing into the receive buffer and completes the pair with MPJX_ERR_ARG on
 *                      every party still waiting (mpjx_last_error names the code and both envelopes; the world stays
 *                      usable; an eager mpjx_send that has returned has returned success). n below the room is legal:
 *                      the first n packed elements of the layout are written, the rest keeps its contents.
 * In a pair with a typed side, that side's buffer must be aligned to its base element (MPJX_ERR_ARG at match).
 * Both on-the-fly kinds are moved by k_wire, one launch per table_max pairs of a claimed batch whatever their
 * directions and layouts, counted in mpjx_comm_p2p_stats' launches too; such a pair is never stored in the segment
 * pool of the persistent requests, and a batch that holds one takes the table path for its other pairs.
 * Status of a receive: a typed receive of a PACKED message has elements = n and bytes = n * word bytes; a PACKED
 * receive of a typed message has bytes = elements = 8 + payload; a PACKED receive of a PACKED message bytes =
 * elements = the bytes sent. mpjx_get_count(status, MPJX_PACKED) treats the size as 1. Sender statuses keep their
 * rule: the sender's own packed bytes. A blocking mpjx_send(PACKED) within the eager limit copies the image into
 * the slab; a typed eager send that meets a PACKED receive is packed on the fly from the slab.
 * mpjx_comm_p2p_wire_stats: for this rank since creation, the k_wire launches, the pairs it packed and unpacked on
 * the fly, and the pairs per launch.
 *
 * mpjx_iprobe: *flag = 1 and *status filled if an unmatched send addressed to this rank, the first in post order,
 * would match a receive (source, tag) posted now; wildcards are honoured, eager sends included. Nothing is consumed
 * and nothing is enqueued on the GPU. mpjx_probe sleeps on the host until there is one, under the bound of every
 * point-to-point wait (MPJX_P2P_TIMEOUT_S / mpjx_comm_set_p2p_timeout): on expiry MPJX_ERR_INTERNAL, and the world
 * is marked failed. The status of a probed message: source, tag, bytes = the sender's packed bytes (image bytes for
 * a PACKED send), elements = bytes / base element bytes, or MPJX_UNDEFINED when the sender used PACKED (the host
 * cannot know the header). mpjx_wire_bytes gives the image a PACKED receive of that message needs: 8 + bytes, or
 * bytes when elements is MPJX_UNDEFINED. A MPJX_PROC_NULL source returns at once with the empty status (flag 1).
 *   MPJX_ERR_ARG: a NULL flag, a bad rank or tag, a NULL communicator, NULL arguments of mpjx_wire_bytes.
 *   MPJX_ERR_UNSUPPORTED: RCCL, IPC and non-direct worlds; for the wait that moves it, a typed layout of 2^32 or
 *   more granules in a pair with PACKED on the other side (as for one message of mpjx_alltoallv_dt). */
int mpjx_iprobe(mpjx_comm_t comm, int source, int tag, int *flag, mpjx_status *status);
int mpjx_probe(mpjx_comm_t comm, int source, int tag, mpjx_status *status);
int mpjx_wire_bytes(const mpjx_status *status, int64_t *bytes);
int mpjx_comm_p2p_wire_stats(mpjx_comm_t comm, int64_t *launches, int64_t *packed, int64_t *unpacked,
                             int *table_max);

/* ---- host-resident variants (Java heap arrays / mpjbuf payloads) ---------------------------------
 * Synchronous. Buffers are ordinary host memory; the library stages them through device memory.
 * These are what the JNI shim calls with GetPrimitiveArrayCritical / GetDirectBufferAddress
 * pointers, replacing the body of nativeReduce (mpjdev_natmpjdev_Intracomm.c:455-623).
 * Host-direct form: in multicore mode with every rank on one device, a call of at most one host
 * pipeline chunk (MPJX_HOST_CHUNK_MIB, default 16 MiB) whose buffers on this rank are page-locked at
 * the same address on the device (mpjx_host_alloc, hipHostMalloc) is not staged: the collective's
 * kernel reads and writes those buffers across the host link. Ranks may mix forms. MPJX_HOST_DIRECT=0
 * turns it off. A buffer qualifies only if its whole byte range lies in ONE such allocation (checked
 * against the allocation's start and size); any other range takes the staged form, whose host copies
 * are split at allocation boundaries. */
int mpjx_reduce_host(mpjx_comm_t comm, const void *sendbuf, void *recvbuf, int64_t count, int type,
                     int op, int root, unsigned flags);
int mpjx_allreduce_host(mpjx_comm_t comm, const void *sendbuf, void *recvbuf, int64_t count, int type,
                        int op, unsigned flags);
int mpjx_reduce_scatter_host(mpjx_comm_t comm, const void *sendbuf, void *recvbuf,
                             const int64_t *recvcounts, int type, int op, unsigned flags);
int mpjx_scan_host(mpjx_comm_t comm, const void *sendbuf, void *recvbuf, int64_t count, int type,
                   int op, unsigned flags);
/* Diagnostic: the form the communicator's last *_host call took on this rank — 1 staged through device
 * buffers (the chunk pipeline), 2 host-direct (the kernel loads and stores the host buffers), 0 none
 * yet. No reference counterpart (tests and latency runs read it). */
int mpjx_comm_last_host_form(mpjx_comm_t comm, int *form);
/* Page-locked host memory the device addresses at the same pointer (hipHostMalloc): staging for a
 * caller whose own arrays cannot stay pinned across a call — the JNI shim's multicore rank threads copy
 * Java arrays through it, so the *_host calls above take their host-direct form. No reference
 * counterpart. mpjx_host_free(NULL) is a no-op. */
int mpjx_host_alloc(void **ptr, int64_t bytes);
int mpjx_host_free(void *ptr);

#ifdef __cplusplus
}
#endif
#endif /* MPJX_H */
