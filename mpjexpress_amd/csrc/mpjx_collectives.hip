// mpjx_collectives.hip — the reduction collectives of libmpjx (Reduce, Allreduce, Reduce_scatter,
// Scan), their companions (Bcast, Gather, Scatter), the block moves (Allgather(v), Gatherv, Scatterv,
// Alltoall(v)) and their form with a derived datatype per side (mpjx_alltoallv_dt), big-endian (mpjbuf)
// payload handling and the host-resident variants, exported through the C ABI declared in include/mpjx.h.
//
// Reference behaviour followed (file:line in /root/reference):
//   Reduce          src/mpi/PureIntracomm.java:1923-1992 (MST_Reduce), :1994-2057 (FT_Reduce)
//   Allreduce       :2168-2185 (Reduce root 0 + MST Bcast), :2187-2314 (FT_Allreduce)
//   Reduce_scatter  :2355-2456 (BKT ring, FT = Reduce + Scatter)
//   Scan            :2495-2545
//   Bcast           :592-736
//   worker tables   src/mpi/<Op>Worker.java (which (op, type) pairs throw MPIException)
// The arithmetic order of each algorithm is reproduced per element by the P-way kernels
// (mpjx_kernels.hpp); the message pattern is replaced by two all-link exchange steps.
#include "mpjx_internal.hpp"
#include "mpjx_kernels_dt.hpp"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <condition_variable>
#include <initializer_list>
#include <mutex>
#include <string>
#include <thread>
#include <utility>

using namespace mpjx;

// ---------------------------------------------------------------------------------------------
// collectives

namespace {

constexpr size_t kAlignBytes = 256;

size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- knobs read from the environment by every call ----

size_t in_slot_skew() {  // MPJX_SLOT_SKEW (bytes, read per call; rounded to 256): input-slot skew (see Slots)
  const char* e = getenv("MPJX_SLOT_SKEW");
  const long v = e ? atol(e) : 0;
  return v > 0 ? ((size_t)v + 255) & ~(size_t)255 : 0;
}

// Small vectors (<= MPJX_ONESHOT_KIB per rank, read per call, default 256): one all-gather of the
// whole vectors and a local P-way combine of all of them, instead of exchange -> combine -> exchange:
// one collective's latency instead of two. Every rank evaluates the same tree, so the bits match.
bool oneshot(size_t bytes) {
  const char* e = getenv("MPJX_ONESHOT_KIB");
  const long kib = e ? atol(e) : 256;
  return kib > 0 && bytes <= ((size_t)kib << 10);
}

// MPJX_PIPE_CHUNK_MIB (read per call): chunk size of the pipelined Allreduce; unset or 0 = off. Off by
// default: on one GPU (configs[4], exchange engine with device copies as transport) it ran 17.8 ms at
// 64 MiB chunks vs 7.7 ms unchunked (profiles/r02/c5_overlap.json) — every chunk adds two collectives'
// fixed cost, and there the "links" are the same HBM the combine streams. The bench times it at N > 1,
// where exchange #1 and the all-gather use different xGMI directions; the 8-GPU run decides.
size_t pipe_chunk_bytes() {
  const char* e = getenv("MPJX_PIPE_CHUNK_MIB");
  long m = e ? atol(e) : 0;
  return m > 0 ? (size_t)m << 20 : 0;
}

size_t host_chunk_bytes() {  // MPJX_HOST_CHUNK_MIB (read per call) overrides the pipeline granularity
  const char* e = getenv("MPJX_HOST_CHUNK_MIB");
  const long m = e ? atol(e) : 0;
  return (size_t)(m > 0 ? m : 16) << 20;
}

bool smp_copy() {  // MPJX_SMP_COPY=1 forces the copy-based exchanges instead of the direct paths
  const char* e = getenv("MPJX_SMP_COPY");
  return e && *e && strcmp(e, "0") != 0;
}

bool host_direct_off() {  // MPJX_HOST_DIRECT=0 turns the *_host calls' host-direct form off
  const char* e = getenv("MPJX_HOST_DIRECT");
  return e && *e && strcmp(e, "0") == 0;
}

// The chunk pipelines' chunk: `want` bytes cut to a multiple of P x 256 B (at least one), so every
// chunk splits into equal, aligned blocks
size_t chunk_bytes(int P, size_t want) {
  const size_t unit = (size_t)P * kAlignBytes;
  return std::max(unit, want / unit * unit);
}

// Per-call context: device, stream ordering against the previous call, scratch.
struct Call {
  mpjx_comm* c;
  hipStream_t s;
  int esz;
  bool blocking = false;  // MPJX_FLAG_BLOCKING: the entry point drains `s` before it returns
  int begin(mpjx_comm* comm, void* stream, int type) {
    c = comm;
    esz = mpjx_type_size(type);
    HIPCHK(hipSetDevice(c->device));
    s = stream ? (hipStream_t)stream : c->stream;
    // an instrumented call that takes a path without marks leaves no phases behind: reading them then
    // fails instead of returning an earlier call's (mpjx_comm_last_phases)
    if (c->phase_on) c->phase_engine = 0;
    if (c->last_stream && c->last_stream != s) {
      if (!c->last_recorded) HIPCHK(hipEventRecord(c->last_ev, c->last_stream));
      HIPCHK(hipStreamWaitEvent(s, c->last_ev, 0));
    }
    return MPJX_SUCCESS;
  }
  // The ordering event is recorded after every call of a multi-rank communicator: a stream whose last
  // command is a cross-stream wait (the direct engine's non-issuing ranks) synchronises 20-30 us
  // slower without it (tools/latency P=4: 35-40 vs 57-79 us per small Allreduce). A one-rank
  // communicator on its OWN stream records it lazily, only when the next call comes on another
  // stream: between back-to-back kernels on one stream the event cost ~3 us per call (allreduce_p1
  // 86.3 vs 83.2 us). A caller-supplied stream gets it at once: the caller may destroy that stream
  // after the call returns, and the next call must not record on it.
  int end() {
    if (blocking) {  // the call returns complete: whatever comes next is ordered after it on the host
      c->last_stream = nullptr;
      c->last_recorded = false;
      return MPJX_SUCCESS;
    }
    c->last_recorded = c->size > 1 || s != c->stream;
    if (c->last_recorded) HIPCHK(hipEventRecord(c->last_ev, s));
    c->last_stream = s;
    return MPJX_SUCCESS;
  }
  int scratch(size_t bytes) { return grow_device(c, &c->scratch, &c->scratch_bytes, bytes, s); }
  // phase boundary i (0..3) of an instrumented call (mpjx_comm_phase_timing); engine: see mpjx_comm
  // (1 exchange: exchange #1 / combine / exchange #2; 2 direct: share / combine / fence; 3 pipelined;
  // 4 one rank: copy; 5 one-shot: all-gather / combine / -; 6 RCCL native: - / ncclAllReduce / -)
  int mark(int i, int engine) {
    if (!c->phase_on) return MPJX_SUCCESS;
    HIPCHK(hipEventRecord(c->phase_ev[i], s));
    c->phase_engine = engine;
    return MPJX_SUCCESS;
  }
};

// Even split of n elements into P blocks whose starts are 256-B aligned (last blocks may be short
// or empty). Block j is reduced by rank j.
struct Blocks {
  std::vector<int64_t> off, len;
  void even(int64_t n, int P, int esz) {
    int64_t a = (int64_t)(kAlignBytes / esz);
    int64_t per = (n + P - 1) / P;
    per = (per + a - 1) / a * a;
    off.resize(P);
    len.resize(P);
    for (int j = 0; j < P; j++) {
      int64_t o = std::min(n, (int64_t)j * per), e = std::min(n, o + per);
      off[j] = o;
      len[j] = e - o;
    }
  }
};

// Scratch layout for one call: P input slots, P output slots, then temporaries.
// Slot placement matters to the P-way kernels: P streams whose addresses are equal modulo a large
// power of two (the natural stride when blocks are 32/64/128 MiB) collide in HBM — cold, K_MST P=8
// over 32 MiB slots runs 50.0 us contiguous vs 47.2 us with slot p shifted by p x 4 KiB, K_SCAN P=8
// 105.7 vs 87.6 us (profiles/r03/slot_skew_cold*.jsonl, tools/slot_skew.py). Output slots are always
// skewed; input slots only when MPJX_SLOT_SKEW says so, because the equal-block exchange #1 needs
// them contiguous for ONE ncclAllToAll (skewed, it becomes an ncclAllToAllv — a trade the 8-GPU run
// measures as the bench variant rccl_skew).
constexpr size_t kSlotSkew = 4096;

struct Slots {
  char* base;
  size_t stride;   // bytes per input slot
  size_t ostride;  // bytes per output slot
  int P;
  char* in(int j) const { return base + (size_t)j * stride; }
  char* out(int j) const { return base + (size_t)P * stride + (size_t)j * ostride; }
  char* tail() const { return base + bytes(); }
  size_t bytes() const { return (size_t)P * (stride + ostride); }
};

Slots make_slots(size_t block_bytes, int P) {
  const size_t r = (block_bytes + kAlignBytes - 1) / kAlignBytes * kAlignBytes;
  return Slots{nullptr, r + in_slot_skew(), r + kSlotSkew, P};
}

size_t temp_bytes(int P, int64_t n, int esz) {
  if (P <= MAXP) return 0;
  int levels = 0;
  for (int m = P; m > MAXP; m = (m + 1) / 2) levels++;
  return (size_t)(2 * levels + 2) * round_up((size_t)n * esz, kAlignBytes);
}

// Scratch for the slots S, the temporaries of an n-element combine behind them (*ts) and `extra` bytes
int carve(Call& k, Slots* S, int64_t n, TempStack* ts, size_t extra = 0) {
  CHK(k.scratch(S->bytes() + temp_bytes(S->P, n, k.esz) + extra));
  S->base = k.c->scratch;
  *ts = TempStack{S->tail(), k.c->scratch_bytes - S->bytes(), 0, (size_t)k.esz};
  return MPJX_SUCCESS;
}

// MPJX_P1_EXCHANGE=1: run world-size-1 Allreduce through the full exchange path (test knob that
// exercises the transport's collective calls on a one-GPU machine).
bool force_exchange() {
  static const bool on = [] {
    const char* e = getenv("MPJX_P1_EXCHANGE");
    return e && *e && strcmp(e, "0") != 0;
  }();
  return on;
}

// MPJX_RCCL_NATIVE=1 (MPJX_RCCL_NATIVE_P2=1: at P = 2 only; read at mpjx_comm_init_rank and checked
// equal on every rank there, RcclTransport::agree): an Allreduce on the RCCL engine whose result cannot
// depend on
// the order the elements are combined in runs as ONE ncclAllReduce instead of exchange -> P-way combine
// -> all-gather. That holds for
//   - byte/int/long SUM, PROD, MAX, MIN at any P: Java's wrap-around integer arithmetic (SumByte's
//     (byte)(a + b), src/mpi/SumByte.java:52; Long multiply modulo 2^64) and signed compares are
//     associative and commutative, so every grouping gives the same bits as MST_Reduce's;
//   - double SUM and PROD at P = 2: the reference's order is ONE operation per element, x1 (op) x0
//     (MST_Reduce root 0, PureIntracomm.java:1943-1992; FT_Allreduce x0 (op) x1, :2187-2314), and IEEE
//     add/multiply are commutative: the same bits in either order, NaN payloads aside (Java does not
//     order those either).
// Not FLOAT: the same argument holds, but whether RCCL's kernels keep binary32 subnormals (Java does;
// a flush-to-zero build would not) has not been checked on a 2-GPU node, so float stays on the
// exchange engine. Not MAX/MIN on floats (Java's `if (in > acc)` keeps a NaN accumulator and the first
// of +0/-0: order matters), not the 16-bit types (RCCL carries no int16/uint16), not pair types, not
// big-endian operands. Off by default: bench.py times it at N <= 2 as a comparison variant beside the
// reported engines (RCCL's own reduction kernel is a ceiling reference, never the reported engine).
bool rccl_native_ok(const RcclTransport* rt, int P, int type, int op, unsigned flags, ncclDataType_t* dt,
                    ncclRedOp_t* ro) {
  // native 2 (MPJX_RCCL_NATIVE_P2=1, VERDICT r4's name for it): the same, at P = 2 only
  if (!rt || !(rt->native == 1 || (rt->native == 2 && P == 2))) return false;
  if (flags & (MPJX_FLAG_SEND_BIG_ENDIAN | MPJX_FLAG_RECV_BIG_ENDIAN)) return false;
  bool integer = true;
  switch (type) {
    case MPJX_BYTE: *dt = ncclInt8; break;
    case MPJX_INT: *dt = ncclInt32; break;
    case MPJX_LONG: *dt = ncclInt64; break;
    case MPJX_DOUBLE: *dt = ncclFloat64; integer = false; break;
    default: return false;
  }
  switch (op) {
    case MPJX_SUM: *ro = ncclSum; break;
    case MPJX_PROD: *ro = ncclProd; break;
    case MPJX_MAX: *ro = ncclMax; break;
    case MPJX_MIN: *ro = ncclMin; break;
    default: return false;
  }
  if (integer) return true;
  return P <= 2 && (op == MPJX_SUM || op == MPJX_PROD);
}

// A rank whose arguments are rejected leaves the collective: tell the transport (IPC marks the world
// so the other ranks' calls fail instead of waiting for this one).
int reject(mpjx_comm* c, int code) {
  if (c && c->tr) c->tr->abort_world();
  return code;
}

// Inside a direct collective (between share() and fence()): a failing step must release the other
// ranks, which are about to wait for this one in fence().
#define DCHK(expr)                              \
  do {                                          \
    int d_ = (expr);                            \
    if (d_ != MPJX_SUCCESS) return reject(c, d_); \
  } while (0)

int check_bufs(mpjx_comm* c, const void* a, const void* b) {
  int rc = check_dev_ptr(a, "buffer");
  if (rc == MPJX_SUCCESS) rc = check_dev_ptr(b, "buffer");
  return rc == MPJX_SUCCESS ? rc : reject(c, rc);
}

// ptrs: also check that the buffers are GPU-accessible (the public device entry points); the *_impl
// bodies (called per window by those) and the host variants validate arguments only.
int validate(mpjx_comm* c, const void* send, const void* recv, int64_t count, int type, int op, bool ptrs = false) {
  if (!c) return fail(MPJX_ERR_ARG, "comm is NULL");
  int rc = mpjx_op_check(op, type);
  if (rc != MPJX_SUCCESS) return reject(c, rc);
  if (count < 0) return reject(c, fail(MPJX_ERR_ARG, "negative count %lld", (long long)count));
  if (count > 0 && (!send || !recv))
    return reject(c, fail(MPJX_ERR_ARG, "NULL buffer with count %lld", (long long)count));
  return count > 0 && ptrs ? check_bufs(c, send, recv) : MPJX_SUCCESS;
}

// exchange #1: block j of `send` -> rank j; rank me receives every peer's block me into in-slot j.
// With equal blocks (the common case: count a multiple of P x 256 B) the own block is copied into its
// slot too so the step is one ncclAllToAll; otherwise the own block is read in place.
bool equal_blocks(const Blocks& B) {
  for (size_t j = 0; j < B.len.size(); j++)
    if (B.len[j] != B.len[0] || B.off[j] != (int64_t)j * B.len[0]) return false;
  return true;
}

int scatter_blocks(Call& k, const char* send, const Blocks& B, const Slots& S, bool* own_in_slot) {
  const int P = k.c->size, me = k.c->rank;
  std::vector<size_t> sc(P), sd(P), rc(P), rd(P);
  const bool eq = equal_blocks(B) && S.stride == (size_t)B.len[0] * k.esz;
  for (int j = 0; j < P; j++) {
    sc[j] = (j == me && !eq) ? 0 : (size_t)B.len[j] * k.esz;
    sd[j] = (size_t)B.off[j] * k.esz;
    rc[j] = (j == me && !eq) ? 0 : (size_t)B.len[me] * k.esz;
    rd[j] = (size_t)j * S.stride;
  }
  *own_in_slot = eq;
  return k.c->tr->alltoallv(me, send, sc, sd, S.in(0), rc, rd, k.s);
}

// exchange #2 (all-gather): my reduced block -> every peer; peers' blocks -> their place in recv
int gather_all_on(Call& k, Transport* tr, hipStream_t s, char* recv, const Blocks& B) {
  const int P = k.c->size, me = k.c->rank;
  if (equal_blocks(B)) return tr->allgather_equal(me, P, recv, (size_t)B.len[0] * k.esz, s);
  std::vector<Xfer> sends, recvs;
  for (int j = 0; j < P; j++) {
    if (j == me) continue;
    if (B.len[me] > 0) sends.push_back({j, recv + B.off[me] * k.esz, (size_t)B.len[me] * k.esz});
    if (B.len[j] > 0) recvs.push_back({j, recv + B.off[j] * k.esz, (size_t)B.len[j] * k.esz});
  }
  return tr->exchange(sends, recvs, s);
}
int gather_all(Call& k, char* recv, const Blocks& B) { return gather_all_on(k, k.c->tr.get(), k.s, recv, B); }

// in[j] = rank j's operand of this rank's block after exchange #1: in-slot j, or `own` (the block in
// the caller's send) where the own block was not copied into its slot
void slot_inputs(const Slots& S, int me, bool own_in_slot, const char* own, std::vector<const void*>* in) {
  in->resize(S.P);
  for (int j = 0; j < S.P; j++) (*in)[j] = (j == me && !own_in_slot) ? (const void*)own : (const void*)S.in(j);
}

// The exchange engine's first half: slots and temporaries in scratch (plan), then exchange #1 and the
// operands of this rank's block (scatter). Two steps, so a caller's phase marks go between them.
struct Exchange {
  Slots S;
  TempStack ts;
  std::vector<const void*> in;
  // slots of slot_elems elements (B.len[0]; Reduce_scatter: its own block, and kAlignBytes `extra`)
  int plan(Call& k, Combine& cb, const Blocks& B, int64_t slot_elems, size_t extra = 0) {
    S = make_slots((size_t)slot_elems * k.esz, k.c->size);
    CHK(carve(k, &S, B.len[k.c->rank], &ts, extra));
    cb.tmp = &ts;
    return MPJX_SUCCESS;
  }
  int scatter(Call& k, const char* send, const Blocks& B) {
    bool own_in_slot = false;
    CHK(scatter_blocks(k, send, B, S, &own_in_slot));
    slot_inputs(S, k.c->rank, own_in_slot, send + B.off[k.c->rank] * k.esz, &in);
    return MPJX_SUCCESS;
  }
};

// Every block back to its rank: out-slot j -> rank j, and block j of `recv` from rank j (the second
// exchange of the plans whose result differs per rank: FT Allreduce, faithful Reduce partials, Scan)
int return_blocks(Call& k, const Slots& S, const Blocks& B, char* recv) {
  const int P = k.c->size, me = k.c->rank;
  std::vector<Xfer> sends, recvs;
  for (int j = 0; j < P; j++) {
    if (j == me) continue;
    if (B.len[me] > 0) sends.push_back({j, S.out(j), (size_t)B.len[me] * k.esz});
    if (B.len[j] > 0) recvs.push_back({j, recv + B.off[j] * k.esz, (size_t)B.len[j] * k.esz});
  }
  return k.c->tr->exchange(sends, recvs, k.s);
}

// A one-rank communicator's call: the copy, between the four phase marks of engine 4
int one_rank_copy(Call& k, Combine& cb, void* recv, const void* send, int64_t n) {
  CHK(k.mark(0, 4));
  CHK(k.mark(1, 4));
  CHK(cb.copy(recv, send, n));
  CHK(k.mark(2, 4));
  CHK(k.mark(3, 4));
  return MPJX_SUCCESS;
}

}  // namespace

namespace {

// ---- direct paths (multicore ranks sharing an address space, or processes mapping each other's
// buffers through HIP IPC): the P-way kernel reads every rank's send block in place and writes its
// result block straight into every rank's recv. One kernel
// and two rendezvous per collective replace exchange #1 + combine + exchange #2 (MPJX_SMP_COPY=1
// forces the copy-based exchanges instead).
Direct* smp_direct(mpjx_comm* c) {
  auto* t = dynamic_cast<Direct*>(c->tr.get());
  return t && t->direct_ok() && !smp_copy() ? t : nullptr;
}

int direct_temps(Call& k, int P, int64_t n, TempStack* ts, int extra = 0) {
  const size_t tb = temp_bytes(P, n, k.esz) + (size_t)extra * round_up((size_t)n * k.esz, kAlignBytes);
  if (tb) CHK(k.scratch(tb));
  *ts = TempStack{k.c->scratch, tb ? k.c->scratch_bytes : 0, 0, (size_t)k.esz};
  return MPJX_SUCCESS;
}

const char* at(const void* base, int64_t elems, int esz) { return (const char*)base + elems * esz; }

// The direct engines' operands from share()'s pointers: in[j] / outs[j] = rank j's send / recv at element
// `off` (outs[j] null where rank j shared no recv: Reduce's non-roots)
void direct_tables(const std::vector<std::vector<const void*>>& all, int64_t off, int esz,
                   std::vector<const void*>* in, std::vector<void*>* outs) {
  const size_t P = all.size();
  in->resize(P);
  outs->resize(P);
  for (size_t j = 0; j < P; j++) {
    (*in)[j] = at(all[j][0], off, esz);
    (*outs)[j] = all[j][1] ? (void*)at(all[j][1], off, esz) : nullptr;
  }
}

// The element range [*off, *off + *n) this rank computes in direct mode: its own block of the even
// partition when the ranks sit on different devices (each GPU's CUs reduce their share), or — all
// ranks on one device — the whole vector on rank 0 and nothing elsewhere: one launch from one
// stream instead of P launches tied together by P·(P−1) cross-stream waits.
void direct_range(int64_t count, int P, int me, int esz, bool lead, int64_t* off, int64_t* n, Parts* parts) {
  Blocks B;
  B.even(count, P, esz);
  parts->off.resize(P);
  parts->len.resize(P);
  for (int j = 0; j < P; j++) {
    parts->off[j] = (size_t)B.off[j] * esz;
    parts->len[j] = (size_t)B.len[j] * esz;
  }
  if (lead) {
    *off = 0;
    *n = (me == 0) ? count : 0;
    return;
  }
  *off = B.off[me];
  *n = B.len[me];
}

// ---- MPJX_FLAG_FAITHFUL buffer side effects (the reference's observable state after the call) ----

// The ranks [*a, *b] whose MST_Reduce partial rank r holds once the reduction is done with it: the
// largest sub-tree r is the root of (PureIntracomm.java:1943-1992 — a rank receives and folds while
// it is the root of its interval, then sends its partial up once as `srce` and stops). The root's
// interval is [0, P-1]. Every rank's recvbuf is the reduction buffer (:1937-1939), so it ends holding
// the MST reduction of its interval.
void mst_subtree(int P, int root, int r, int* a, int* b) {
  int l = 0, h = P - 1, rt = root;
  while (r != rt) {
    const int mid = (l + h) / 2;
    const int srce = (rt <= mid) ? h : l;
    if (r <= mid) {
      rt = (rt <= mid) ? rt : srce;
      h = mid;
    } else {
      rt = (rt > mid) ? rt : srce;
      l = mid + 1;
    }
  }
  *a = l;
  *b = h;
}

// out[r] (r < P, null = skip) = range `n` of rank r's MST partial, from range `n` of every rank's send
// (in[]). With `via_tmp` the results go through temporaries first (some out[r] aliases an in[j]).
// `last` (>= 0): the one rank whose out may alias its own in (the exchange engine: out[me] is the
// caller's recv, in[me] its send, the same memory in place); its partial is computed after every other
// partial has read in[last], and reads in[last] element by element before storing over it, so no
// temporaries are needed.
int mst_partials(Combine& cb, const std::vector<const void*>& in, const std::vector<void*>& out, int root,
                 int64_t n, bool via_tmp, int last = -1) {
  const int P = (int)in.size();
  std::vector<void*> res(out);
  if (via_tmp)
    for (int r = 0; r < P; r++)
      if (out[r] && !(res[r] = cb.tmp->push(n)))
        return fail(MPJX_ERR_INTERNAL, "scratch temporaries exhausted (faithful Reduce, P=%d)", P);
  for (int i = 0; i < P; i++) {
    const int r = (last < 0) ? i : (last + 1 + i) % P;  // `last` comes last
    if (!out[r]) continue;
    int a, b;
    mst_subtree(P, root, r, &a, &b);
    if (via_tmp) {  // native temporary, converted to the recv byte order by the copy below
      CHK(cb.mst_o(in.data(), a, b, r, res[r], false, n));
    } else {
      CHK(cb.mst(in.data(), a, b, r, res[r], n));
    }
  }
  if (via_tmp)
    for (int r = 0; r < P; r++)
      if (out[r]) CHK(cb.copy_o(out[r], res[r], n, cb.rbe()));
  return MPJX_SUCCESS;
}

// BKT_Reduce_scatter (P >= 2) stores its arr into the caller's sendbuf every round
// (getResultant(buf, offset, count), PureIntracomm.java:2427-2428): afterwards block `me` holds the
// rank's result and every other element its own value with the zero tmpbuf folded in P-1 times
// (:2409 createTemporaryBuffer is zero-filled). Runs after every peer has read this rank's send.
int bkt_sendbuf(Call& k, Combine& cb, char* send, int64_t total, int64_t boff, int64_t n, const char* recv_block,
                int P) {
  if (total <= 0) return MPJX_SUCCESS;
  CHK(cb.copy_o(send + boff * k.esz, recv_block, n, cb.sbe() != cb.rbe()));
  const int64_t zmax = std::max<int64_t>(1, (int64_t)((size_t)16 << 20) / k.esz);
  const int64_t zn = std::min(zmax, std::max(boff, total - boff - n));
  if (zn <= 0) return MPJX_SUCCESS;
  CHK(k.scratch((size_t)zn * k.esz));
  HIPCHK(hipMemsetAsync(k.c->scratch, 0, (size_t)zn * k.esz, k.s));
  const int64_t seg[2][2] = {{0, boff}, {boff + n, total}};
  for (const auto& sg : seg)
    for (int64_t o = sg[0]; o < sg[1]; o += zn)
      CHK(cb.zero_fold(send + o * k.esz, k.c->scratch, P - 1, std::min(zn, sg[1] - o)));
  return MPJX_SUCCESS;
}

}  // namespace

namespace {

// The one-shot engines' scratch: P slots of one whole vector each (slot j = rank j's), then temporaries
int oneshot_slots(Call& k, int64_t count, Slots* S, TempStack* ts) {
  *S = Slots{nullptr, round_up((size_t)count * k.esz, kAlignBytes), 0, k.c->size};  // input slots only
  return carve(k, S, count, ts);
}

// Gather every rank's whole send vector into the one-shot slots; in[j] = rank j's vector.
int oneshot_gather(Call& k, const void* send, int64_t count, std::vector<const void*>* in, TempStack* ts) {
  mpjx_comm* c = k.c;
  const int P = c->size, me = c->rank;
  Slots S;
  CHK(oneshot_slots(k, count, &S, ts));
  HIPCHK(hipMemcpyAsync(S.in(me), send, (size_t)count * k.esz, hipMemcpyDeviceToDevice, k.s));
  CHK(c->tr->allgather_equal(me, P, S.base, S.stride, k.s));
  in->resize(P);
  for (int j = 0; j < P; j++) (*in)[j] = S.in(j);
  return MPJX_SUCCESS;
}

// Chunked Allreduce (default MST order) on three streams: exchange #1 of every chunk on the call's
// stream, chunk k's P-way combine on the communicator's combine stream once its exchange #1 is in, and
// chunk k's all-gather on the gather stream once its combine is done — through the transport's SECOND
// lane (RCCL: a second communicator, since RCCL serialises one communicator's operations whatever
// their streams). So exchange #1 of chunk k+1, the combine of chunk k and the all-gather of chunk k-1
// can all be in flight at once, each on its own resource (outbound scatter, HBM, inbound gather). The
// op is element-wise: every chunk reduces exactly as the whole vector would, so the results are
// bit-identical to the unchunked call.
int allreduce_pipelined(Call& k, const char* send, char* recv, int64_t count, int64_t ce, int op, int type,
                        unsigned flags) {
  mpjx_comm* c = k.c;
  const int P = c->size, me = c->rank;
  const int64_t nch = (count + ce - 1) / ce;
  Blocks B0;
  B0.even(ce, P, k.esz);
  const size_t stride = round_up((size_t)B0.len[0] * k.esz, kAlignBytes);
  const size_t per_chunk = (size_t)P * stride;
  CHK(k.scratch((size_t)nch * per_chunk + temp_bytes(P, B0.len[0], k.esz)));
  if (!c->cstream) HIPCHK(hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
  if (!c->gstream) HIPCHK(hipStreamCreateWithFlags(&c->gstream, hipStreamNonBlocking));
  Transport* g2 = c->tr->lane2();
  if (!g2) return fail(MPJX_ERR_RCCL, "the pipeline's second exchange lane is unavailable");
  while (c->pipe_ev.size() < (size_t)(2 * nch + 2)) {
    hipEvent_t e;
    HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->pipe_ev.push_back(e);
  }
  hipEvent_t ev_start = c->pipe_ev[2 * nch], ev_done = c->pipe_ev[2 * nch + 1];
  TempStack ts{c->scratch + (size_t)nch * per_chunk, c->scratch_bytes - (size_t)nch * per_chunk, 0, (size_t)k.esz};
  Combine cb{op, type, flags, k.esz, c->cstream, &ts};
  CHK(k.mark(0, 3));
  // phase timing on: timing events at every chunk's interval boundaries (mpjx_comm_pipeline_trace)
  const bool tr = c->phase_on;
  if (tr) {
    while (c->trace_ev.size() < (size_t)(1 + 6 * nch)) {
      hipEvent_t e;
      HIPCHK(hipEventCreate(&e));
      c->trace_ev.push_back(e);
    }
    c->trace_chunks = (int)nch;
    HIPCHK(hipEventRecord(c->trace_ev[0], k.s));
  }
  auto tev = [&](int64_t ch, int i, hipStream_t st) -> int {
    if (tr) HIPCHK(hipEventRecord(c->trace_ev[1 + 6 * ch + i], st));
    return MPJX_SUCCESS;
  };
  // the gather stream starts after everything before this call on the call's stream (recv's last users)
  HIPCHK(hipEventRecord(ev_start, k.s));
  HIPCHK(hipStreamWaitEvent(c->gstream, ev_start, 0));
  Blocks prev;
  int64_t prev_off = 0;
  std::vector<const void*> in(P);
  for (int64_t ch = 0; ch < nch; ch++) {
    const int64_t off = ch * ce, len = std::min(ce, count - off);
    Blocks B;
    B.even(len, P, k.esz);
    Slots S{c->scratch + (size_t)ch * per_chunk, stride, stride, P};  // input slots only
    bool own_in_slot = false;
    CHK(tev(ch, 0, k.s));
    CHK(scatter_blocks(k, send + off * k.esz, B, S, &own_in_slot));  // exchange #1 (chunk ch), call stream
    CHK(tev(ch, 1, k.s));
    hipEvent_t ev_in = c->pipe_ev[2 * ch], ev_out = c->pipe_ev[2 * ch + 1];
    HIPCHK(hipEventRecord(ev_in, k.s));
    HIPCHK(hipStreamWaitEvent(c->cstream, ev_in, 0));
    slot_inputs(S, me, own_in_slot, send + (off + B.off[me]) * k.esz, &in);
    CHK(tev(ch, 2, c->cstream));
    CHK(cb.mst(in.data(), 0, P - 1, 0, recv + (off + B.off[me]) * k.esz, B.len[me]));  // combine (chunk ch)
    CHK(tev(ch, 3, c->cstream));
    HIPCHK(hipEventRecord(ev_out, c->cstream));
    if (ch > 0) {  // exchange #2 of the previous chunk, after its combine, on the second lane
      HIPCHK(hipStreamWaitEvent(c->gstream, c->pipe_ev[2 * ch - 1], 0));
      CHK(tev(ch - 1, 4, c->gstream));
      CHK(gather_all_on(k, g2, c->gstream, recv + prev_off * k.esz, prev));
      CHK(tev(ch - 1, 5, c->gstream));
    }
    prev = B;
    prev_off = off;
  }
  HIPCHK(hipStreamWaitEvent(c->gstream, c->pipe_ev[2 * nch - 1], 0));
  CHK(tev(nch - 1, 4, c->gstream));
  CHK(gather_all_on(k, g2, c->gstream, recv + prev_off * k.esz, prev));
  CHK(tev(nch - 1, 5, c->gstream));
  HIPCHK(hipEventRecord(ev_done, c->gstream));
  HIPCHK(hipStreamWaitEvent(k.s, ev_done, 0));
  CHK(k.mark(3, 3));
  return k.end();
}

}  // namespace

static int mpjx_allreduce_impl(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type,
                              int op, unsigned flags, void* stream) {
  CHK(validate(c, sendbuf, recvbuf, count, type, op));
  Call k;
  CHK(k.begin(c, stream, type));
  k.blocking = (flags & MPJX_FLAG_BLOCKING) != 0;
  const int P = c->size, me = c->rank;
  const char* send = (const char*)sendbuf;
  char* recv = (char*)recvbuf;
  if (count == 0) return k.end();
  Combine cb{op, type, flags, k.esz, k.s, nullptr};
  if (P == 1 && !force_exchange()) {  // Reduce = arraycopy(send -> recv) (:1937); Bcast = nothing
    CHK(one_rank_copy(k, cb, recv, send, count));
    return k.end();
  }
  ncclDataType_t ndt;
  ncclRedOp_t nro;
  auto* rt = dynamic_cast<RcclTransport*>(c->tr.get());
  if (rccl_native_ok(rt, P, type, op, flags, &ndt, &nro)) {  // one ncclAllReduce (see rccl_native_ok)
    CHK(k.mark(0, 6));
    CHK(k.mark(1, 6));
    CHK(rt->allreduce(send, recv, (size_t)count, ndt, nro, k.s));
    CHK(k.mark(2, 6));
    CHK(k.mark(3, 6));
    return k.end();
  }
  if (Direct* t = smp_direct(c)) {
    const bool lead = t->single();
    int64_t off, n;
    Parts parts;
    direct_range(count, P, me, k.esz, lead, &off, &n, &parts);
    TempStack ts;
    CHK(direct_temps(k, P, n, &ts, (flags & MPJX_FLAG_OLD_COLLECTIVES) ? P : 0));
    cb.tmp = &ts;
    std::vector<std::vector<const void*>> all;
    CHK(k.mark(0, 2));
    CHK(t->share(sendbuf, (size_t)count * k.esz, recvbuf, (size_t)count * k.esz, parts, k.s, &all, lead));
    DCHK(k.mark(1, 2));
    std::vector<const void*> in;
    std::vector<void*> outs;
    direct_tables(all, off, k.esz, &in, &outs);
    bool signalled = false;  // the IPC device-sync fence flag stored from the combine kernel's tail
    if (n == 0) {
    } else if (!(flags & MPJX_FLAG_OLD_COLLECTIVES)) {
      unsigned long long tseq = 0;
      if (P <= MAXP) cb.arm_tail(t->tail_arm((size_t)count * k.esz, &tseq), tseq);  // one launch: mst_rep
      // MST(0) range -> every rank's recv
      const int rc = cb.mst_rep(in.data(), P, 0, outs.data(), P, n);
      signalled = cb.disarm_tail();
      DCHK(rc);
    } else {
      // FT_Allreduce: rank r's own fold order for rank r's recv. An in-place rank's recv block is an
      // input of every later fold, so results go through temporaries until all folds are done.
      bool alias = false;
      for (int j = 0; j < P; j++) alias |= (all[j][0] == all[j][1]);
      std::vector<void*> res(outs);
      if (alias) {
        for (int r = 0; r < P; r++)
          if (!(res[r] = ts.push(n))) return reject(c, fail(MPJX_ERR_INTERNAL, "scratch temporaries exhausted (P=%d)", P));
      }
      for (int r = 0; r < P; r++) DCHK(cb.ft(in.data(), P, r, res[r], n));
      if (alias)
        for (int r = 0; r < P; r++) DCHK(cb.copy_raw(outs[r], res[r], n));
    }
    DCHK(k.mark(2, 2));
    CHK(t->fence(k.s, lead, signalled, (flags & MPJX_FLAG_BLOCKING) != 0));
    CHK(k.mark(3, 2));
    return k.end();
  }
  if (oneshot((size_t)count * k.esz)) {
    TempStack ts;
    std::vector<const void*> in;
    CHK(k.mark(0, 5));
    CHK(oneshot_gather(k, sendbuf, count, &in, &ts));
    CHK(k.mark(1, 5));
    cb.tmp = &ts;
    if (!(flags & MPJX_FLAG_OLD_COLLECTIVES)) {
      CHK(cb.mst(in.data(), 0, P - 1, 0, recv, count));
    } else {  // FT_Allreduce: this rank's own order
      CHK(cb.ft(in.data(), P, me, recv, count));
    }
    CHK(k.mark(2, 5));
    CHK(k.mark(3, 5));
    return k.end();
  }
  if (!(flags & MPJX_FLAG_OLD_COLLECTIVES)) {
    const size_t pcb = pipe_chunk_bytes();
    const int64_t ce = pcb ? (int64_t)(chunk_bytes(P, pcb) / k.esz) : 0;
    if (ce > 0 && count > ce) return allreduce_pipelined(k, send, recv, count, ce, op, type, flags);
  }
  Blocks B;
  B.even(count, P, k.esz);
  const int64_t n = B.len[me];
  Exchange x;
  CHK(x.plan(k, cb, B, B.len[0]));
  CHK(k.mark(0, 1));
  CHK(x.scatter(k, send, B));
  CHK(k.mark(1, 1));
  char* mine = recv + B.off[me] * k.esz;
  if (!(flags & MPJX_FLAG_OLD_COLLECTIVES)) {
    // MST_Reduce to root 0 then MST_Bcast: one result, the root-0 tree order, on every rank
    CHK(cb.mst(x.in.data(), 0, P - 1, 0, mine, n));
    CHK(k.mark(2, 1));
    CHK(gather_all(k, recv, B));
  } else {
    // FT_Allreduce: rank r starts from x_r and folds the others in ascending order — a different
    // order per rank, so rank me computes block me of EVERY rank's result and returns them.
    for (int r = 0; r < P; r++) CHK(cb.ft(x.in.data(), P, r, r == me ? (void*)mine : (void*)x.S.out(r), n));
    CHK(k.mark(2, 1));
    CHK(return_blocks(k, x.S, B, recv));
  }
  CHK(k.mark(3, 1));
  return k.end();
}

static int mpjx_reduce_impl(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type,
                           int op, int root, unsigned flags, void* stream) {
  if (!c) return fail(MPJX_ERR_ARG, "comm is NULL");
  CHK(check_root(c, root));
  // recvbuf is significant at the root only — and on every rank under MPJX_FLAG_FAITHFUL, where it is
  // left as the reference leaves it (MST: the rank's sub-tree partial; FT: its own send copy)
  const bool faithful = (flags & MPJX_FLAG_FAITHFUL) != 0, old = (flags & MPJX_FLAG_OLD_COLLECTIVES) != 0;
  CHK(validate(c, sendbuf, (c->rank == root || faithful) ? recvbuf : sendbuf, count, type, op));
  Call k;
  CHK(k.begin(c, stream, type));
  k.blocking = (flags & MPJX_FLAG_BLOCKING) != 0;
  const int P = c->size, me = c->rank;
  const char* send = (const char*)sendbuf;
  char* recv = (char*)recvbuf;
  if (count == 0) return k.end();
  Combine cb{op, type, flags, k.esz, k.s, nullptr};
  // FT_Reduce (:2038,2052) ends with getResultant(recvbuf) on every rank: a non-root's recvbuf gets
  // the copy of its own send that createInitialBuffer made
  auto finish = [&]() -> int {
    if (faithful && old && me != root) CHK(cb.copy(recv, send, count));
    return k.end();
  };
  if (P == 1) {
    CHK(cb.copy(recv, send, count));
    return k.end();
  }
  Blocks B;
  B.even(count, P, k.esz);
  const int64_t n = B.len[me];
  const bool partials = faithful && !old;  // every rank's recv gets its MST sub-tree partial
  if (Direct* t = smp_direct(c)) {
    const bool lead = t->single();
    int64_t doff, dn;
    Parts parts;
    direct_range(count, P, me, k.esz, lead, &doff, &dn, &parts);
    std::vector<std::vector<const void*>> all;
    CHK(t->share(sendbuf, (size_t)count * k.esz, recvbuf, (me == root || partials) ? (size_t)count * k.esz : 0, parts,
                 k.s, &all, lead));
    bool alias = false;
    for (int j = 0; j < P; j++) alias |= partials && all[j][1] && all[j][0] == all[j][1];
    TempStack dts;
    DCHK(direct_temps(k, P, dn, &dts, alias ? P : 0));
    cb.tmp = &dts;
    std::vector<const void*> in;
    std::vector<void*> outs;  // outs[root]: straight into the root's recv
    direct_tables(all, doff, k.esz, &in, &outs);
    if (dn == 0) {
    } else if (partials) {
      DCHK(mst_partials(cb, in, outs, root, dn, alias));
    } else if (!old) {
      DCHK(cb.mst(in.data(), 0, P - 1, root, outs[root], dn));
    } else {
      DCHK(cb.ft(in.data(), P, root, outs[root], dn));
    }
    CHK(t->fence(k.s, lead, false, (flags & MPJX_FLAG_BLOCKING) != 0));
    return finish();
  }
  if (!partials && oneshot((size_t)count * k.esz)) {  // small: every whole vector to the root, which reduces them all
    const size_t bytes = (size_t)count * k.esz;
    std::vector<Xfer> sends, recvs;
    if (me != root) {
      sends.push_back({root, (void*)sendbuf, bytes});
      CHK(c->tr->exchange(sends, recvs, k.s));
      return finish();
    }
    Slots S;
    TempStack ots;
    CHK(oneshot_slots(k, count, &S, &ots));
    cb.tmp = &ots;
    std::vector<const void*> in(P);
    for (int j = 0; j < P; j++) {
      in[j] = (j == me) ? sendbuf : (const void*)S.in(j);
      if (j != me) recvs.push_back({j, S.in(j), bytes});
    }
    CHK(c->tr->exchange(sends, recvs, k.s));
    if (!old) {
      CHK(cb.mst(in.data(), 0, P - 1, root, recv, count));
    } else {
      CHK(cb.ft(in.data(), P, root, recv, count));
    }
    return k.end();
  }
  Exchange x;
  CHK(x.plan(k, cb, B, B.len[0]));
  CHK(x.scatter(k, send, B));
  if (partials) {
    // block me of every rank's partial, then each block to its rank (the exchange Scan uses)
    std::vector<void*> outs(P);
    for (int j = 0; j < P; j++) outs[j] = (j == me) ? (void*)(recv + B.off[me] * k.esz) : (void*)x.S.out(j);
    CHK(mst_partials(cb, x.in, outs, root, n, false, me));  // outs[me] may alias in[me] (in place)
    CHK(return_blocks(k, x.S, B, recv));
    return k.end();
  }
  void* out = (me == root) ? (void*)(recv + B.off[me] * k.esz) : (void*)x.S.out(0);
  if (!old) {
    CHK(cb.mst(x.in.data(), 0, P - 1, root, out, n));  // MST_Reduce rooted at `root`
  } else {
    CHK(cb.ft(x.in.data(), P, root, out, n));  // FT_Reduce: x_root, then ranks 0..P-1 (skipping root) folded in
  }
  // gather the reduced blocks at the root
  std::vector<Xfer> sends, recvs;
  if (me != root) {
    if (n > 0) sends.push_back({root, out, (size_t)n * k.esz});
  } else {
    for (int j = 0; j < P; j++)
      if (j != root && B.len[j] > 0) recvs.push_back({j, recv + B.off[j] * k.esz, (size_t)B.len[j] * k.esz});
  }
  CHK(c->tr->exchange(sends, recvs, k.s));
  return finish();
}

static int mpjx_reduce_scatter_impl(mpjx_comm_t c, const void* sendbuf, void* recvbuf,
                                   const int64_t* recvcounts, int type, int op, unsigned flags,
                                   void* stream) {
  if (!c) return fail(MPJX_ERR_ARG, "comm is NULL");
  if (!recvcounts) return fail(MPJX_ERR_ARG, "recvcounts is NULL");
  const int P = c->size, me = c->rank;
  Blocks B;
  B.off.resize(P);
  B.len.resize(P);
  int64_t total = 0;
  for (int j = 0; j < P; j++) {
    if (recvcounts[j] < 0) return fail(MPJX_ERR_ARG, "recvcounts[%d] < 0", j);
    B.off[j] = total;
    B.len[j] = recvcounts[j];
    total += recvcounts[j];
  }
  CHK(validate(c, sendbuf, B.len[me] > 0 ? recvbuf : sendbuf, total, type, op));
  Call k;
  CHK(k.begin(c, stream, type));
  k.blocking = (flags & MPJX_FLAG_BLOCKING) != 0;
  const char* send = (const char*)sendbuf;
  char* recv = (char*)recvbuf;
  const int64_t n = B.len[me];
  Combine cb{op, type, flags, k.esz, k.s, nullptr};
  if (P == 1) {
    CHK(one_rank_copy(k, cb, recv, send, n));
    return k.end();
  }
  // MPJX_FLAG_FAITHFUL: the BKT ring (default collectives, typed ops) leaves its arr in sendbuf
  const bool bkt_send = (flags & MPJX_FLAG_FAITHFUL) && !(flags & MPJX_FLAG_OLD_COLLECTIVES) && !is_pair(type);
  if (Direct* t = smp_direct(c)) {
    // block r of the result goes to rank r: this rank computes its own block, or (one device) rank 0
    // computes every block
    const bool lead = t->single();
    const int lo = lead ? 0 : me, hi = lead ? (me == 0 ? P : 0) : me + 1;
    int64_t nmax = 0;
    for (int r = lo; r < hi; r++) nmax = std::max(nmax, B.len[r]);
    TempStack dts;
    CHK(direct_temps(k, P, nmax, &dts));
    cb.tmp = &dts;
    std::vector<std::vector<const void*>> all;
    Parts parts;
    for (int j = 0; j < P; j++) {
      parts.off.push_back((size_t)B.off[j] * k.esz);
      parts.len.push_back((size_t)B.len[j] * k.esz);
    }
    CHK(k.mark(0, 2));
    CHK(t->share(sendbuf, (size_t)total * k.esz, recvbuf, (size_t)B.len[me] * k.esz, parts, k.s, &all, lead));
    DCHK(k.mark(1, 2));
    std::vector<const void*> in(P);
    bool signalled = false;
    for (int r = lo; r < hi; r++) {
      const int64_t nr = B.len[r];
      void* out = (void*)all[r][1];
      for (int j = 0; j < P; j++) in[j] = at(all[j][0], B.off[r], k.esz);
      unsigned long long tseq = 0;  // one combine launch per rank (P <= 8, not the lead mode)
      if (!lead && P <= MAXP) cb.arm_tail(t->tail_arm((size_t)total * k.esz, &tseq), tseq);
      if (nr == 0) {
      } else if (flags & MPJX_FLAG_OLD_COLLECTIVES) {
        DCHK(cb.fold(P, in.data(), out, nr));
      } else if (P <= 2 && !is_pair(type)) {
        const void* lst[2] = {in[r], in[(r + 1) % P]};
        DCHK(cb.fold(2, lst, out, nr));
      } else if ((flags & MPJX_FLAG_FAITHFUL) && !is_pair(type)) {
        DCHK(cb.bkt(in[r], in[(r + 1) % P], P - 1, out, nr));
      } else {
        DCHK(cb.mst(in.data(), 0, P - 1, 0, out, nr));
      }
      signalled = cb.disarm_tail() || signalled;
    }
    DCHK(k.mark(2, 2));
    CHK(t->fence(k.s, lead, signalled, (flags & MPJX_FLAG_BLOCKING) != 0));
    CHK(k.mark(3, 2));
    if (bkt_send) CHK(bkt_sendbuf(k, cb, (char*)sendbuf, total, B.off[me], n, recv, P));
    return k.end();
  }
  Exchange x;
  CHK(x.plan(k, cb, B, n, kAlignBytes));  // slots of this rank's own block: the blocks differ in size
  CHK(k.mark(0, 1));
  CHK(x.scatter(k, send, B));
  CHK(k.mark(1, 1));
  const std::vector<const void*>& in = x.in;
  if (flags & MPJX_FLAG_OLD_COLLECTIVES) {
    // FT_Reduce_scatter = FT_Reduce(root 0) + Scatter: x_0 folded with x_1 .. x_{P-1}
    CHK(cb.fold(P, in.data(), recv, n));
  } else if (P <= 2 && !is_pair(type)) {
    // BKT_Reduce_scatter, P=2: acc = own block, the successor's block folded in once
    const void* lst[2] = {in[me], in[(me + 1) % P]};
    CHK(cb.fold(2, lst, recv, n));
  } else if ((flags & MPJX_FLAG_FAITHFUL) && !is_pair(type)) {
    // the reference's P>=3 ring (defect A9): own block and the successor's copy of it, P-1 rounds
    CHK(cb.bkt(in[me], in[(me + 1) % P], P - 1, recv, n));
  } else {
    // MPI-correct result for P>=3: block me of Reduce(root 0) in the MST order
    CHK(cb.mst(in.data(), 0, P - 1, 0, recv, n));
  }
  CHK(k.mark(2, 1));
  if (bkt_send) CHK(bkt_sendbuf(k, cb, (char*)sendbuf, total, B.off[me], n, recv, P));
  CHK(k.mark(3, 1));  // no exchange #2 (the faithful sendbuf rewrite, if any, is timed here)
  return k.end();
}

static int mpjx_scan_impl(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type,
                         int op, unsigned flags, void* stream) {
  CHK(validate(c, sendbuf, recvbuf, count, type, op));
  Call k;
  CHK(k.begin(c, stream, type));
  k.blocking = (flags & MPJX_FLAG_BLOCKING) != 0;
  const int P = c->size, me = c->rank;
  const char* send = (const char*)sendbuf;
  char* recv = (char*)recvbuf;
  if (count == 0) return k.end();
  Combine cb{op, type, flags, k.esz, k.s, nullptr};
  if (P == 1) {
    CHK(one_rank_copy(k, cb, recv, send, count));
    return k.end();
  }
  Blocks B;
  B.even(count, P, k.esz);
  const int64_t n = B.len[me];
  if (Direct* t = smp_direct(c)) {
    const bool lead = t->single();
    int64_t doff, dn;
    Parts parts;
    direct_range(count, P, me, k.esz, lead, &doff, &dn, &parts);
    TempStack dts;
    CHK(direct_temps(k, P, dn, &dts));
    cb.tmp = &dts;
    std::vector<std::vector<const void*>> all;
    CHK(k.mark(0, 2));
    CHK(t->share(sendbuf, (size_t)count * k.esz, recvbuf, (size_t)count * k.esz, parts, k.s, &all, lead));
    DCHK(k.mark(1, 2));
    std::vector<const void*> in;
    std::vector<void*> outs;  // this range of rank j's prefix -> rank j
    direct_tables(all, doff, k.esz, &in, &outs);
    unsigned long long tseq = 0;  // one K_SCAN launch at P <= 8
    if (P <= MAXP) cb.arm_tail(t->tail_arm((size_t)count * k.esz, &tseq), tseq);
    const int src = cb.scan(P, in.data(), outs.data(), dn);
    const bool signalled = cb.disarm_tail();
    DCHK(src);
    DCHK(k.mark(2, 2));
    CHK(t->fence(k.s, lead, signalled, (flags & MPJX_FLAG_BLOCKING) != 0));
    CHK(k.mark(3, 2));
    return k.end();
  }
  if (oneshot((size_t)count * k.esz)) {  // x_{me-1} (op) (... (op) (x_0 (op) x_me)) from the gathered vectors
    TempStack ots;
    std::vector<const void*> all;
    CHK(k.mark(0, 5));
    CHK(oneshot_gather(k, sendbuf, count, &all, &ots));
    CHK(k.mark(1, 5));
    cb.tmp = &ots;
    CHK(cb.prefix(all.data(), me, recv, count));
    CHK(k.mark(2, 5));
    CHK(k.mark(3, 5));
    return k.end();
  }
  Exchange x;
  CHK(x.plan(k, cb, B, B.len[0]));
  CHK(k.mark(0, 1));
  CHK(x.scatter(k, send, B));
  CHK(k.mark(1, 1));
  std::vector<void*> out(P);
  for (int j = 0; j < P; j++) out[j] = (j == me) ? (void*)(recv + B.off[me] * k.esz) : (void*)x.S.out(j);
  // block me of every rank's prefix, each in the reference's fold order
  CHK(cb.scan(P, x.in.data(), out.data(), n));
  CHK(k.mark(2, 1));
  CHK(return_blocks(k, x.S, B, recv));
  CHK(k.mark(3, 1));
  return k.end();
}

static int bcast_entry(mpjx_comm_t c, void* buf, int64_t count, int type, int root, void* stream) {
  if (!c) return fail(MPJX_ERR_ARG, "comm is NULL");
  if (mpjx_type_size(type) == 0) return fail(MPJX_ERR_ARG, "unknown datatype code %d", type);
  CHK(check_root(c, root));
  if (count < 0 || (count > 0 && !buf)) return reject(c, fail(MPJX_ERR_ARG, "bad buffer/count"));
  if (count > 0) CHK(check_bufs(c, buf, nullptr));
  Call k;
  CHK(k.begin(c, stream, type));
  const int P = c->size, me = c->rank;
  if (count == 0 || P == 1) return k.end();
  char* b = (char*)buf;
  Blocks B;
  B.even(count, P, k.esz);
  // scatter from the root, then every non-root block owner shares its block with the non-roots
  std::vector<Xfer> sends, recvs;
  if (me == root) {
    for (int j = 0; j < P; j++)
      if (j != root && B.len[j] > 0) sends.push_back({j, b + B.off[j] * k.esz, (size_t)B.len[j] * k.esz});
  } else if (B.len[me] > 0) {
    recvs.push_back({root, b + B.off[me] * k.esz, (size_t)B.len[me] * k.esz});
  }
  CHK(c->tr->exchange(sends, recvs, k.s));
  sends.clear();
  recvs.clear();
  for (int j = 0; j < P; j++) {
    if (j == me) continue;
    if (me == root) {  // the root's own block goes to every other rank
      if (B.len[root] > 0) sends.push_back({j, b + B.off[root] * k.esz, (size_t)B.len[root] * k.esz});
    } else if (j != root) {  // non-roots share the block they got from the root
      if (B.len[me] > 0) sends.push_back({j, b + B.off[me] * k.esz, (size_t)B.len[me] * k.esz});
      if (B.len[j] > 0) recvs.push_back({j, b + B.off[j] * k.esz, (size_t)B.len[j] * k.esz});
    }
  }
  if (me != root && B.len[root] > 0)
    recvs.push_back({root, b + B.off[root] * k.esz, (size_t)B.len[root] * k.esz});
  CHK(c->tr->exchange(sends, recvs, k.s));
  return k.end();
}

static int gather_entry(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, int root,
                        void* stream) {
  if (!c) return fail(MPJX_ERR_ARG, "comm is NULL");
  if (mpjx_type_size(type) == 0) return fail(MPJX_ERR_ARG, "unknown datatype code %d", type);
  CHK(check_root(c, root));
  if (count < 0 || (count > 0 && (!sendbuf || (c->rank == root && !recvbuf))))
    return reject(c, fail(MPJX_ERR_ARG, "bad buffer/count"));
  if (count > 0) CHK(check_bufs(c, sendbuf, c->rank == root ? recvbuf : nullptr));
  Call k;
  CHK(k.begin(c, stream, type));
  const size_t nb = (size_t)count * k.esz;
  if (nb == 0) return k.end();
  std::vector<Xfer> sends, recvs;
  if (c->rank == root) {
    char* r = (char*)recvbuf;
    HIPCHK(hipMemcpyAsync(r + (size_t)root * nb, sendbuf, nb, hipMemcpyDeviceToDevice, k.s));
    for (int j = 0; j < c->size; j++)
      if (j != root) recvs.push_back({j, r + (size_t)j * nb, nb});
  } else {
    sends.push_back({root, (void*)sendbuf, nb});
  }
  CHK(c->tr->exchange(sends, recvs, k.s));
  return k.end();
}

static int scatter_entry(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, int root,
                         void* stream) {
  if (!c) return fail(MPJX_ERR_ARG, "comm is NULL");
  if (mpjx_type_size(type) == 0) return fail(MPJX_ERR_ARG, "unknown datatype code %d", type);
  CHK(check_root(c, root));
  if (count < 0 || (count > 0 && (!recvbuf || (c->rank == root && !sendbuf))))
    return reject(c, fail(MPJX_ERR_ARG, "bad buffer/count"));
  if (count > 0) CHK(check_bufs(c, recvbuf, c->rank == root ? sendbuf : nullptr));
  Call k;
  CHK(k.begin(c, stream, type));
  const size_t nb = (size_t)count * k.esz;
  if (nb == 0) return k.end();
  std::vector<Xfer> sends, recvs;
  if (c->rank == root) {
    const char* sb = (const char*)sendbuf;
    HIPCHK(hipMemcpyAsync(recvbuf, sb + (size_t)root * nb, nb, hipMemcpyDeviceToDevice, k.s));
    for (int j = 0; j < c->size; j++)
      if (j != root) sends.push_back({j, (void*)(sb + (size_t)j * nb), nb});
  } else {
    recvs.push_back({root, recvbuf, nb});
  }
  CHK(c->tr->exchange(sends, recvs, k.s));
  return k.end();
}

// ---------------------------------------------------------------------------------------------
// byte order: big-endian (mpjbuf) send/recv buffers are swapped inside the combine kernels (Combine,
// mpjx_internal.hpp): exchanges move the send bytes raw, every P-way kernel swaps its operands in
// registers after the load and its results before the store. No separate pass over the vector.

namespace {
// Elements one direct-path call may cover: the IPC engine stages through a fixed region, so longer
// vectors run as consecutive windows (every collective here is element-wise, so a window reduces
// exactly as the whole vector would: same bits). Unlimited for the other engines.
int64_t window_elems(mpjx_comm* c, int type) {
  Direct* t = smp_direct(c);
  const size_t w = t ? t->window_bytes() : SIZE_MAX;
  const int esz = mpjx_type_size(type);
  return (w == SIZE_MAX || esz == 0) ? INT64_MAX : std::max<int64_t>(1, (int64_t)(w / esz));
}
const char* cadv(const void* p, int64_t elems, int type) {
  return p ? (const char*)p + elems * mpjx_type_size(type) : nullptr;
}
}  // namespace

namespace {
// MPJX_FLAG_BLOCKING reaches only a call's last window (earlier windows stay asynchronous, ordered by
// the call's stream); the entry point then drains the call's stream, so the call returns complete.
unsigned window_flags(unsigned flags, bool last) { return last ? flags : flags & ~MPJX_FLAG_BLOCKING; }

int finish_blocking(mpjx_comm* c, unsigned flags, void* stream) {
  if (!(flags & MPJX_FLAG_BLOCKING)) return MPJX_SUCCESS;
  return c->tr->wait(stream ? (hipStream_t)stream : c->stream);
}

// An element-wise collective over its windows: impl(send, recv, count, flags) once per window (once for
// an empty call), then the blocking call's drain
template <class Fn>
int windowed(mpjx_comm* c, const void* sendbuf, void* recvbuf, int64_t count, int type, unsigned flags, void* stream,
             Fn impl) {
  HIPCHK(hipSetDevice(c->device));
  const int64_t we = window_elems(c, type);
  for (int64_t off = 0; off < count || off == 0; off += we)
    CHK(impl(cadv(sendbuf, off, type), (void*)cadv(recvbuf, off, type), std::min(we, count - off),
             window_flags(flags, off + we >= count)));
  return finish_blocking(c, flags, stream);
}
}  // namespace

static int allreduce_entry(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, int op,
                           unsigned flags, void* stream) {
  CHK(validate(c, sendbuf, recvbuf, count, type, op, true));
  return windowed(c, sendbuf, recvbuf, count, type, flags, stream, [&](const void* s, void* r, int64_t n, unsigned f) {
    return mpjx_allreduce_impl(c, s, r, n, type, op, f, stream);
  });
}

static int reduce_entry(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, int op,
                        int root, unsigned flags, void* stream) {
  if (!c) return fail(MPJX_ERR_ARG, "comm is NULL");
  CHK(check_root(c, root));
  const bool all_recv = c->rank == root || (flags & MPJX_FLAG_FAITHFUL);
  CHK(validate(c, sendbuf, all_recv ? recvbuf : sendbuf, count, type, op, true));
  return windowed(c, sendbuf, recvbuf, count, type, flags, stream, [&](const void* s, void* r, int64_t n, unsigned f) {
    return mpjx_reduce_impl(c, s, r, n, type, op, root, f, stream);
  });
}

static int reduce_scatter_entry(mpjx_comm_t c, const void* sendbuf, void* recvbuf, const int64_t* recvcounts,
                                int type, int op, unsigned flags, void* stream) {
  if (!c) return fail(MPJX_ERR_ARG, "comm is NULL");
  // a rank without recvcounts leaves the collective: multicore/IPC peers are released, not left waiting
  if (!recvcounts) return reject(c, fail(MPJX_ERR_ARG, "recvcounts is NULL"));
  int64_t total = 0;
  for (int j = 0; j < c->size; j++) total += recvcounts[j] > 0 ? recvcounts[j] : 0;
  CHK(check_bufs(c, total > 0 ? sendbuf : nullptr, recvcounts[c->rank] > 0 ? recvbuf : nullptr));
  const void* s2 = sendbuf;
  HIPCHK(hipSetDevice(c->device));
  const int64_t we = window_elems(c, type);
  if (total <= we) {
    CHK(mpjx_reduce_scatter_impl(c, s2, recvbuf, recvcounts, type, op, flags, stream));
  } else {  // windows over the whole vector; rank j's share of a window is its block's overlap with it
    const int P = c->size, me = c->rank;
    std::vector<int64_t> boff(P), rc(P);
    for (int j = 0, o = 0; j < P; j++) { boff[j] = o; o += recvcounts[j] > 0 ? recvcounts[j] : 0; }
    for (int64_t w = 0; w < total; w += we) {
      const int64_t w1 = std::min(total, w + we);
      for (int j = 0; j < P; j++) {
        const int64_t end = boff[j] + (recvcounts[j] > 0 ? recvcounts[j] : 0);
        rc[j] = std::max<int64_t>(0, std::min(w1, end) - std::max(w, boff[j]));
      }
      void* r = (void*)cadv(recvbuf, rc[me] > 0 ? std::max(w, boff[me]) - boff[me] : 0, type);
      CHK(mpjx_reduce_scatter_impl(c, cadv(s2, w, type), r, rc.data(), type, op, window_flags(flags, w1 >= total),
                                   stream));
    }
  }
  return finish_blocking(c, flags, stream);
}

static int scan_entry(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, int op,
                      unsigned flags, void* stream) {
  CHK(validate(c, sendbuf, recvbuf, count, type, op, true));
  return windowed(c, sendbuf, recvbuf, count, type, flags, stream, [&](const void* s, void* r, int64_t n, unsigned f) {
    return mpjx_scan_impl(c, s, r, n, type, op, f, stream);
  });
}

extern "C" int mpjx_comm_phase_timing(mpjx_comm_t c, int enable) {
  COMM_ARG(c);
  HIPCHK(hipSetDevice(c->device));
  for (hipEvent_t& e : c->phase_ev)
    if (!e) HIPCHK(hipEventCreate(&e));
  c->phase_on = enable != 0;
  c->phase_engine = 0;
  return MPJX_SUCCESS;
}

extern "C" int mpjx_comm_last_phases(mpjx_comm_t c, float* ms3, int* engine) {
  COMM_ARG(c);
  if (!ms3 || !engine) return fail(MPJX_ERR_ARG, "NULL argument");
  *engine = c->phase_engine;
  ms3[0] = ms3[1] = ms3[2] = -1.0f;
  if (!c->phase_engine) return fail(MPJX_ERR_ARG, "the last call with phase timing on recorded no phases (none yet, or a path without marks)");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipEventSynchronize(c->phase_ev[3]));
  if (c->phase_engine == 3) {  // pipelined: the chunks' phases overlap; only the whole call
    HIPCHK(hipEventElapsedTime(&ms3[0], c->phase_ev[0], c->phase_ev[3]));
    return MPJX_SUCCESS;
  }
  for (int i = 0; i < 3; i++) HIPCHK(hipEventElapsedTime(&ms3[i], c->phase_ev[i], c->phase_ev[i + 1]));
  return MPJX_SUCCESS;
}

extern "C" int mpjx_comm_pipeline_trace(mpjx_comm_t c, float* ms, int cap, int* nchunks) {
  COMM_ARG(c);
  if (!ms || !nchunks || cap < 0) return fail(MPJX_ERR_ARG, "bad arguments");
  *nchunks = 0;
  if (c->phase_engine != 3 || !c->trace_chunks)
    return fail(MPJX_ERR_ARG, "the last instrumented Allreduce was not chunk-pipelined");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipEventSynchronize(c->phase_ev[3]));
  const int n = std::min(c->trace_chunks, cap / 6);
  for (int i = 0; i < 6 * n; i++) HIPCHK(hipEventElapsedTime(&ms[i], c->trace_ev[0], c->trace_ev[1 + i]));
  *nchunks = n;
  return MPJX_SUCCESS;
}

extern "C" int mpjx_mpjbuf_section(const void* buf, int64_t nbytes, int64_t pos, int* type, int64_t* count,
                                   int64_t* data_pos) {
  if (!buf || !type || !count || !data_pos || pos < 0 || nbytes < 0) return fail(MPJX_ERR_ARG, "bad arguments");
  const int64_t h = (pos + 7) / 8 * 8;  // ALIGNMENT_UNIT
  if (h + 8 > nbytes) return fail(MPJX_ERR_ARG, "section header at %lld past the end (%lld bytes)", (long long)h,
                                  (long long)nbytes);
  const unsigned char* b = (const unsigned char*)buf + h;
  const int code = b[0];
  if (code > 7)
    return fail(MPJX_ERR_UNSUPPORTED, "mpjbuf section type %d is not a static primitive section", code);
  const int64_t n = (int64_t)(((uint32_t)b[4] << 24) | ((uint32_t)b[5] << 16) | ((uint32_t)b[6] << 8) | b[7]);
  const int t = code + 1;
  if (h + 8 + n * mpjx_type_size(t) > nbytes) return fail(MPJX_ERR_ARG, "section payload overruns the buffer");
  *type = t;
  *count = n;
  *data_pos = h + 8;
  return MPJX_SUCCESS;
}

// ---------------------------------------------------------------------------------------------
// host-resident variants
//
// Host arrays (Java heap arrays pinned by the JNI shim, mpjbuf direct buffers) are staged through
// device buffers held by the communicator. Element-wise collectives (Allreduce, Reduce, Scan) are
// chunk-pipelined: the calling thread copies chunk c+1 host->device while the device runs the
// collective on chunk c and a second thread drains chunk c-1 device->host, so both PCIe directions
// and the collective overlap (full duplex). Every rank walks the chunks in the same order.

namespace {
int host_stage(Call& k, size_t bytes) { return grow_device(k.c, &k.c->hstage, &k.c->hstage_bytes, bytes, k.s); }

// The allocation holding p (page-locked host memory, hipHostMalloc'd or hipHostRegister'ed, or device
// memory): [*start, *start + *size), or false for pageable memory. hipPointerGetAttribute's RANGE_START_ADDR
// and RANGE_SIZE give the extent the runtime's own copy validation uses, for allocated and registered memory
// alike; hipMemGetAddressRange reports no base for registered memory (profiles/r06/probe_host_f.jsonl).
bool alloc_range(const void* p, const char** start, size_t* size) {
  void* s = nullptr;
  size_t z = 0;
  if (hipPointerGetAttribute(&s, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, (hipDeviceptr_t)p) != hipSuccess ||
      hipPointerGetAttribute(&z, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, (hipDeviceptr_t)p) != hipSuccess || !s || !z) {
    (void)hipGetLastError();  // pageable memory: the query fails, and must not leave a sticky error
    return false;
  }
  const char* q = (const char*)p;
  if (q < (const char*)s || q >= (const char*)s + z) return false;
  *start = (const char*)s;
  *size = z;
  return true;
}

// [p, p + bytes) lies inside ONE allocation (checked against the allocation's start and size).
bool in_one_allocation(const void* p, size_t bytes) {
  const char* s = nullptr;
  size_t z = 0;
  return alloc_range(p, &s, &z) && bytes <= z - (size_t)((const char*)p - s);
}

// hipMemcpyAsync between device memory and a host range, in pieces that each lie inside one page-locked
// allocation, or start in pageable memory (the runtime's pageable path; at most one host chunk each, each
// piece's start looked up again): a host range that starts in one page-locked allocation and runs on past
// its end is not one copy the runtime takes (hipErrorInvalidValue, probe_host_f.jsonl). The usual range is
// one piece (one lookup per copy).
hipError_t host_copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s) {
  const char* h = (const char*)(kind == hipMemcpyHostToDevice ? src : dst);
  const size_t pageable_piece = (size_t)16 << 20;
  for (size_t done = 0; done < bytes;) {
    const char* q = h + done;
    const char* as = nullptr;
    size_t az = 0;
    const size_t seg = alloc_range(q, &as, &az) ? std::min(bytes - done, (size_t)(as + az - q))
                                                : std::min(bytes - done, pageable_piece);
    const hipError_t e = hipMemcpyAsync((char*)dst + done, (const char*)src + done, seg, kind, s);
    if (e != hipSuccess) return e;
    done += seg;
  }
  return hipSuccess;
}

// [p, p + bytes) is page-locked host memory inside ONE allocation; `identity`: and the device addresses
// it at the same pointer
bool host_locked(const void* p, size_t bytes, bool identity) {
  hipPointerAttribute_t a{};
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory: the query fails, and must not leave a sticky error
    return false;
  }
  return a.type == hipMemoryTypeHost && (!identity || a.devicePointer == p) && in_one_allocation(p, bytes);
}

bool host_pinned(const void* p, size_t bytes) { return host_locked(p, bytes, false); }

// [p, p + bytes) is page-locked host memory the device addresses at the same pointer (hipHostMalloc'd,
// e.g. through mpjx_host_alloc), inside ONE allocation: a kernel can load and store it as it is.
// hipHostRegister'ed memory whose device alias differs does not qualify. The whole range is checked
// against the allocation's own start and size: a range that starts in one page-locked
// block and ends in another, with pageable or unmapped memory between, passed a first-and-last-byte
// check and would have reached a kernel as a GPU fault; it now takes the staged form.
bool host_identity_mapped(const void* p, size_t bytes) { return host_locked(p, bytes, true); }

// The host-direct form of the *_host calls (round 5). Multicore mode with every rank on ONE device (the
// direct engine's single-launch form), a call that is one host-pipeline chunk on every rank (count <=
// chunk elements: the same answer everywhere), and this rank's buffers page-locked at the same address
// on the device: the buffers go to the device entry point as they are, and rank 0's one P-way kernel
// reads every rank's operands and writes every rank's results across the host link (kernel loads and
// stores of page-locked memory run 57 GB/s one way and 45.7 each way both at once,
// profiles/r05/tuning/pcie_probe_l.jsonl) — no H2D, D2H or device staging. Every rank still makes
// exactly one collective call, so a rank whose buffers are pageable (staged) and a rank taking this form
// meet in the same direct call. The JNI shim's multicore staging is page-locked for this reason.
// MPJX_HOST_DIRECT=0 turns it off.
bool host_direct_ok(mpjx_comm* c, int64_t count, int type, std::initializer_list<std::pair<const void*, size_t>> bufs) {
  if (host_direct_off()) return false;
  Direct* t = smp_direct(c);
  if (!t || !t->single()) return false;
  const size_t esz = (size_t)mpjx_type_size(type);
  if (!esz || count > (int64_t)(chunk_bytes(c->size, host_chunk_bytes()) / esz)) return false;
  for (const auto& b : bufs)
    if (b.first && b.second && !host_identity_mapped(b.first, b.second)) return false;
  return true;
}

// Chunk-pipelined host collective. Chunk c moves host -> device on the H2D stream, runs the
// collective fn(dsend, drecv, count, stream) on the call's stream and moves back on the D2H stream, so
// both directions of the host link and the collective overlap. A pageable destination is drained by
// a second thread (a pageable copy returns only when it is done, so it must not hold up the thread
// that issues the next chunks); a page-locked one is copied straight from the issuing thread. Every
// rank walks the chunks in the same order.
//
// Measured at P = 1, 256 MiB (tools/e2e_bench.py, profiles/r04/e2e_host_z3.json): 42.9-43.8 GB/s of S/t
// from pageable arrays, 44.7 from page-locked ones at the default 16 MiB chunks — the 44 GB/s the same
// chunk chain reaches with bare copies (tools/tuning/pcie_probe.hip "pipeline dma"); two unchunked DMA
// copies at once run 48.4 GB/s each way. The copy streams and events are the communicator's: creating
// them in every call cost 4-5 GB/s (39 vs 43.7 GB/s, the same run). Page-locked arrays with 8 MiB chunks
// run 30-34 GB/s (issued all at once, 32 blit copies queue behind the collectives); 16 and 32 MiB do not.
// Staging pageable chunks through a pinned ring with 4-8 host copy threads per direction was slower
// (21-37 GB/s: the host copies and the DMA compete, profiles/r04/e2e_host_m.json) and is not used.
template <class Fn>
int host_pipeline(mpjx_comm* c, const void* sendbuf, void* recvbuf, int64_t count, int type, bool out_here,
                  Fn fn) {
  Call k;
  CHK(k.begin(c, nullptr, type));
  const size_t esz = (size_t)k.esz, bytes = (size_t)count * esz, half = round_up(bytes, kAlignBytes);
  CHK(host_stage(k, 2 * half + kAlignBytes));
  char *ds = c->hstage, *dr = c->hstage + half;
  const size_t cb = chunk_bytes(c->size, host_chunk_bytes());
  const int64_t ce = (int64_t)(cb / esz);
  const int64_t nchunks = (count + ce - 1) / ce;
  if (nchunks <= 1) {  // small: one chunk, on the call's stream
    HIPCHK(host_copy(ds, sendbuf, bytes, hipMemcpyHostToDevice, k.s));
    CHK(fn(ds, dr, count, k.s));
    if (out_here) HIPCHK(host_copy(recvbuf, dr, bytes, hipMemcpyDeviceToHost, k.s));
    CHK(k.c->tr->wait(k.s));
    return k.end();
  }
  const bool pin_out = out_here && host_pinned(recvbuf, bytes);
  const size_t ne = (size_t)nchunks;
  // the communicator's copy streams and per-chunk events (kept between calls: every earlier call has
  // drained them before it returned; each event keeps its role, recorded on the same stream every call)
  if (!c->h2d) HIPCHK(hipStreamCreateWithFlags(&c->h2d, hipStreamNonBlocking));
  if (!c->d2h) HIPCHK(hipStreamCreateWithFlags(&c->d2h, hipStreamNonBlocking));
  for (auto* v : {&c->host_in_ev, &c->host_coll_ev})
    while (v->size() < ne) {
      hipEvent_t e = nullptr;
      HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      v->push_back(e);
    }
  hipStream_t h2d = c->h2d, d2h = c->d2h;
  const hipEvent_t* in_ev = c->host_in_ev.data();
  const hipEvent_t* coll_ev = c->host_coll_ev.data();
  auto chunk = [&](int64_t ch, size_t* off, size_t* nb) {
    *off = (size_t)ch * cb;
    *nb = std::min(bytes - *off, cb);
  };
  std::mutex mu;
  std::condition_variable cv;
  int64_t issued = 0;  // chunks whose collective is enqueued (guarded by mu)
  bool abort = false;
  std::string drain_err;
  const int dev = c->device;
  std::thread drain;
  if (out_here && !pin_out)
    drain = std::thread([&]() {
      (void)hipSetDevice(dev);
      for (int64_t ch = 0; ch < nchunks; ch++) {
        {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [&] { return issued > ch || abort; });
          if (issued <= ch) return;  // aborted before this chunk was issued
        }
        size_t off, nb;
        chunk(ch, &off, &nb);
        hipError_t e = hipStreamWaitEvent(d2h, coll_ev[ch], 0);
        if (e == hipSuccess) e = host_copy((char*)recvbuf + off, dr + off, nb, hipMemcpyDeviceToHost, d2h);
        if (e == hipSuccess) e = hipStreamSynchronize(d2h);
        if (e != hipSuccess) {
          std::lock_guard<std::mutex> lk(mu);
          drain_err = hipGetErrorString(e);
          return;
        }
      }
    });
  int rc = MPJX_SUCCESS;
  for (int64_t ch = 0; ch < nchunks && rc == MPJX_SUCCESS; ch++) {
    size_t off, nb;
    chunk(ch, &off, &nb);
    hipError_t e = host_copy(ds + off, (const char*)sendbuf + off, nb, hipMemcpyHostToDevice, h2d);
    if (e == hipSuccess) e = hipEventRecord(in_ev[ch], h2d);
    if (e == hipSuccess) e = hipStreamWaitEvent(k.s, in_ev[ch], 0);
    if (e != hipSuccess) {
      rc = fail(MPJX_ERR_HIP, "H2D chunk: %s", hipGetErrorString(e));
      break;
    }
    rc = fn(ds + off, dr + off, (int64_t)(nb / esz), k.s);
    if (rc == MPJX_SUCCESS && hipEventRecord(coll_ev[ch], k.s) != hipSuccess) rc = fail(MPJX_ERR_HIP, "event record");
    if (rc != MPJX_SUCCESS) break;
    if (pin_out) {  // page-locked destination: straight back on the D2H stream
      e = hipStreamWaitEvent(d2h, coll_ev[ch], 0);
      if (e == hipSuccess) e = host_copy((char*)recvbuf + off, dr + off, nb, hipMemcpyDeviceToHost, d2h);
      if (e != hipSuccess) rc = fail(MPJX_ERR_HIP, "D2H chunk: %s", hipGetErrorString(e));
    }
    {
      std::lock_guard<std::mutex> lk(mu);
      issued = ch + 1;
    }
    cv.notify_all();
  }
  {
    std::lock_guard<std::mutex> lk(mu);
    if (rc != MPJX_SUCCESS) abort = true;
  }
  cv.notify_all();
  // wait on the collective stream first: over RCCL this polls for asynchronous errors and the
  // MPJX_RCCL_TIMEOUT_S limit, and an abort releases the kernels the drain thread's copies wait on
  const int wrc = c->tr->wait(k.s);
  {
    std::lock_guard<std::mutex> lk(mu);
    abort = true;  // nothing more will be issued
  }
  cv.notify_all();
  if (drain.joinable()) drain.join();
  hipError_t se = hipStreamSynchronize(h2d);  // every issued copy is done before the events are reused
  if (se == hipSuccess) se = hipStreamSynchronize(d2h);
  if (rc != MPJX_SUCCESS) return rc;
  if (wrc != MPJX_SUCCESS) return wrc;
  if (!drain_err.empty()) return fail(MPJX_ERR_HIP, "D2H chunk: %s", drain_err.c_str());
  if (se != hipSuccess) return fail(MPJX_ERR_HIP, "host pipeline: %s", hipGetErrorString(se));
  return k.end();
}

// An element-wise *_host call, arguments validated: the host-direct form — call(send, recv, count, flags,
// stream) on the host buffers, blocking — if this rank's buffers qualify, else the chunk pipeline over
// `call`. out_here: recvbuf is significant on this rank.
template <class Fn>
int host_call(mpjx_comm* c, const void* sendbuf, void* recvbuf, int64_t count, int type, unsigned flags, bool out_here,
              Fn call) {
  if (count == 0) return MPJX_SUCCESS;
  const size_t bytes = (size_t)count * mpjx_type_size(type);
  void* out = out_here ? recvbuf : nullptr;
  if (host_direct_ok(c, count, type, {{sendbuf, bytes}, {out, bytes}})) {
    c->host_form = 2;
    return call(sendbuf, out, count, flags | MPJX_FLAG_BLOCKING, nullptr);
  }
  c->host_form = 1;
  return host_pipeline(c, sendbuf, recvbuf, count, type, out_here, [&](char* ds, char* dr, int64_t n, hipStream_t s) {
    return call(ds, dr, n, flags, s);
  });
}
}  // namespace

extern "C" int mpjx_host_alloc(void** ptr, int64_t bytes) {
  if (!ptr || bytes < 0) return fail(MPJX_ERR_ARG, "mpjx_host_alloc: bad argument");
  *ptr = nullptr;
  HIPCHK(hipHostMalloc(ptr, (size_t)std::max<int64_t>(bytes, 1), hipHostMallocDefault));
  return MPJX_SUCCESS;
}

extern "C" int mpjx_host_free(void* ptr) {
  if (ptr) HIPCHK(hipHostFree(ptr));
  return MPJX_SUCCESS;
}

static int allreduce_host_entry(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type,
                                int op, unsigned flags) {
  flags &= ~MPJX_FLAG_BLOCKING;  // synchronous anyway; the chunks' collectives must stay asynchronous
  CHK(validate(c, sendbuf, recvbuf, count, type, op));
  return host_call(c, sendbuf, recvbuf, count, type, flags, true,
                   [&](const void* s, void* r, int64_t n, unsigned f, void* stream) {
                     return mpjx_allreduce(c, s, r, n, type, op, f, stream);
                   });
}

static int reduce_host_entry(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type,
                             int op, int root, unsigned flags) {
  flags &= ~MPJX_FLAG_BLOCKING;  // synchronous anyway; the chunks' collectives must stay asynchronous
  if (!c) return fail(MPJX_ERR_ARG, "comm is NULL");
  CHK(check_root(c, root));
  const bool all_recv = c->rank == root || (flags & MPJX_FLAG_FAITHFUL);  // faithful: every rank's recvbuf
  CHK(validate(c, sendbuf, all_recv ? recvbuf : sendbuf, count, type, op));
  return host_call(c, sendbuf, recvbuf, count, type, flags, all_recv,
                   [&](const void* s, void* r, int64_t n, unsigned f, void* stream) {
                     return mpjx_reduce(c, s, r, n, type, op, root, f, stream);
                   });
}

static int scan_host_entry(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type,
                           int op, unsigned flags) {
  flags &= ~MPJX_FLAG_BLOCKING;  // synchronous anyway; the chunks' collectives must stay asynchronous
  CHK(validate(c, sendbuf, recvbuf, count, type, op));
  return host_call(c, sendbuf, recvbuf, count, type, flags, true,
                   [&](const void* s, void* r, int64_t n, unsigned f, void* stream) {
                     return mpjx_scan(c, s, r, n, type, op, f, stream);
                   });
}

static int reduce_scatter_host_entry(mpjx_comm_t c, const void* sendbuf, void* recvbuf,
                                     const int64_t* recvcounts, int type, int op, unsigned flags) {
  flags &= ~MPJX_FLAG_BLOCKING;  // synchronous anyway; the chunks' collectives must stay asynchronous
  if (!c) return fail(MPJX_ERR_ARG, "comm is NULL");
  // a rank without recvcounts leaves the collective: multicore/IPC peers are released, not left waiting
  if (!recvcounts) return reject(c, fail(MPJX_ERR_ARG, "recvcounts is NULL"));
  int64_t total = 0;
  for (int j = 0; j < c->size; j++) total += recvcounts[j] > 0 ? recvcounts[j] : 0;
  const int64_t mine = recvcounts[c->rank];
  CHK(validate(c, sendbuf, mine > 0 ? recvbuf : sendbuf, total, type, op));
  const size_t esz = (size_t)mpjx_type_size(type);
  if (total > 0 && host_direct_ok(c, total, type, {{sendbuf, (size_t)total * esz}, {recvbuf, (size_t)std::max<int64_t>(mine, 0) * esz}})) {
    c->host_form = 2;
    return mpjx_reduce_scatter(c, sendbuf, mine > 0 ? recvbuf : nullptr, recvcounts, type, op,
                               flags | MPJX_FLAG_BLOCKING, nullptr);
  }
  c->host_form = 1;
  Call k;
  CHK(k.begin(c, nullptr, type));
  size_t bytes = (size_t)total * k.esz, half = round_up(bytes, kAlignBytes);
  CHK(host_stage(k, half + round_up((size_t)mine * k.esz, kAlignBytes) + kAlignBytes));
  char *ds = c->hstage, *dr = c->hstage + half;
  HIPCHK(host_copy(ds, sendbuf, bytes, hipMemcpyHostToDevice, k.s));
  CHK(k.end());
  CHK(mpjx_reduce_scatter(c, ds, dr, recvcounts, type, op, flags, k.s));
  if (mine > 0) HIPCHK(host_copy(recvbuf, dr, (size_t)mine * k.esz, hipMemcpyDeviceToHost, k.s));
  // faithful BKT ring (P >= 2): the staged sendbuf was rewritten as the reference rewrites the caller's
  if ((flags & MPJX_FLAG_FAITHFUL) && !(flags & MPJX_FLAG_OLD_COLLECTIVES) && !is_pair(type) && c->size >= 2 &&
      bytes > 0)
    HIPCHK(host_copy((void*)sendbuf, ds, bytes, hipMemcpyDeviceToHost, k.s));
  CHK(k.c->tr->wait(k.s));
  return MPJX_SUCCESS;
}

extern "C" int mpjx_comm_last_host_form(mpjx_comm_t c, int* form) {
  COMM_ARG(c);
  if (!form) return fail(MPJX_ERR_ARG, "NULL argument");
  *form = c->host_form;
  return MPJX_SUCCESS;
}

// ---------------------------------------------------------------------------------------------
// block moves: Allgather, Allgatherv, Gatherv, Scatterv, Alltoall, Alltoallv
// (src/mpi/Intracomm.java:363-690 -> PureIntracomm.java). Plain bytes: no op, no byte order. Each call
// is, per rank, P send ranges (S[j]: what goes to rank j) and P receive ranges (R[j]: what comes from
// rank j) in bytes from its two buffers (planned and validated by mpjx_moves_plan.hpp), then one of
// three engines:
//   P = 1                     one k_moves launch (never hipMemcpyAsync)
//   multicore, one device     every rank publishes its buffers and ranges (share), rank 0 launches
//                             k_moves over the whole world's <= P x P segments, every rank fences: one
//                             kernel and two rendezvous per call, like the reductions. Every rank sees
//                             every table there, so a send length that differs from the matching
//                             receive length is MPJX_ERR_ARG on every rank before any launch.
//   every other world         the rank's own block by k_moves, the rest through the transport
//                             (allgather_equal / alltoallv / exchange), where matching counts are the
//                             caller's contract as in MPI. Multicore ranks on distinct devices take this
//                             path too: a one-launch kernel over peer memory has no machine to be tested on.

namespace {

struct MovePlan {
  const char* send;
  char* recv;
  std::vector<ByteRange> S, R;
};

enum MoveKind { MV_ALLGATHER, MV_ALLTOALL, MV_EXCHANGE };

int plan_fail(const std::string& err) { return fail(MPJX_ERR_ARG, "%s", err.c_str()); }

// p->X[at] = `count` elements at offset 0, every other entry empty (n entries)
int plan_single(std::vector<ByteRange>* x, int n, int at, int64_t count, int esz, const char* what) {
  std::vector<ByteRange> one;
  std::string err;
  if (!plan_ranges(&count, nullptr, 1, esz, &one, &err, what)) return plan_fail(err);
  x->assign((size_t)n, ByteRange{0, 0});
  if (at >= 0) (*x)[(size_t)at] = one[0];
  else x->assign((size_t)n, one[0]);  // at < 0: the same range for every rank
  return MPJX_SUCCESS;
}

int plan_table(std::vector<ByteRange>* x, int n, const int64_t* counts, const int64_t* displs, int esz,
               const char* what) {
  if (!counts || !displs) return fail(MPJX_ERR_ARG, "%s or their displacements are NULL", what);
  std::string err;
  if (!plan_ranges(counts, displs, n, esz, x, &err, what)) return plan_fail(err);
  return MPJX_SUCCESS;
}

int moves_check(mpjx_comm* c, const MovePlan& p) {
  int64_t st = 0, rt = 0;
  for (const ByteRange& x : p.S) st += x.len;
  for (const ByteRange& x : p.R) rt += x.len;
  if ((st > 0 && !p.send) || (rt > 0 && !p.recv)) return fail(MPJX_ERR_ARG, "NULL buffer with a nonzero count");
  CHK(check_bufs(c, st > 0 ? p.send : nullptr, rt > 0 ? p.recv : nullptr));
  int a = 0, b = 0;
  if (ranges_overlap(p.R, &a, &b))
    return fail(MPJX_ERR_ARG, "the receive segments from ranks %d and %d overlap", a, b);
  if (ranges_cross((uint64_t)(uintptr_t)p.send, p.S, (uint64_t)(uintptr_t)p.recv, p.R))
    return fail(MPJX_ERR_ARG, "send and receive ranges overlap (these collectives have no in-place form)");
  return MPJX_SUCCESS;
}

int own_mismatch(int me, const MovePlan& p) {
  return fail(MPJX_ERR_ARG, "rank %d sends itself %lld bytes but receives %lld", me, (long long)p.S[me].len,
              (long long)p.R[me].len);
}

int moves_run(mpjx_comm* c, MoveKind kind, MovePlan& p, int type, void* stream) {
  c->move_kernels = 0;
  CHK(moves_check(c, p));
  Call k;
  CHK(k.begin(c, stream, type));
  const int P = c->size, me = c->rank;
  if (p.S[me].len != p.R[me].len) return own_mismatch(me, p);
  auto* t = dynamic_cast<SmpTransport*>(c->tr.get());
  if (P > 1 && t && smp_direct(c) && t->single()) {
    // The ranges stay in this rank's frame: no rank leaves the call before the fence's rendezvous
    std::vector<std::vector<const void*>> all;
    CHK(t->share(std::vector<const void*>{p.send, p.recv, &p.S, &p.R}, k.s, &all, true));
    auto S = [&](int i) -> const std::vector<ByteRange>& { return *(const std::vector<ByteRange>*)all[i][2]; };
    auto R = [&](int i) -> const std::vector<ByteRange>& { return *(const std::vector<ByteRange>*)all[i][3]; };
    for (int i = 0; i < P; i++)
      for (int j = 0; j < P; j++)
        if (S(i)[j].len != R(j)[i].len) {
          const long long sl = S(i)[j].len, rl = R(j)[i].len;
          (void)t->fence(k.s, true);  // every rank has read every table before any rank returns
          return fail(MPJX_ERR_ARG, "rank %d sends %lld bytes to rank %d, which receives %lld", i, sl, j, rl);
        }
    if (me == 0) {
      MoveList ml;
      for (int j = 0; j < P; j++)    // receiver
        for (int i = 0; i < P; i++)  // sender
          ml.add((char*)all[j][1] + R(j)[i].off, (const char*)all[i][0] + S(i)[j].off, R(j)[i].len);
      if (!ml.segs.empty()) c->move_kernels |= MPJX_MOVE_KERNEL_MOVES;
      HIPCHK(launch_moves(ml, k.s));
    }
    CHK(t->fence(k.s, true));
    return k.end();
  }
  {
    MoveList ml;
    ml.add(p.recv + p.R[me].off, p.send + p.S[me].off, p.R[me].len);
    if (!ml.segs.empty()) c->move_kernels |= MPJX_MOVE_KERNEL_MOVES;
    HIPCHK(launch_moves(ml, k.s));
  }
  if (P == 1) return k.end();
  if (kind == MV_ALLGATHER) {
    CHK(c->tr->allgather_equal(me, P, p.recv, (size_t)p.R[me].len, k.s));
  } else if (kind == MV_ALLTOALL) {
    std::vector<size_t> sc(P), sd(P), rc(P), rd(P);
    for (int j = 0; j < P; j++) {
      sc[j] = j == me ? 0 : (size_t)p.S[j].len;
      sd[j] = (size_t)p.S[j].off;
      rc[j] = j == me ? 0 : (size_t)p.R[j].len;
      rd[j] = (size_t)p.R[j].off;
    }
    CHK(c->tr->alltoallv(me, p.send, sc, sd, p.recv, rc, rd, k.s));
  } else {
    std::vector<Xfer> sends, recvs;
    for (int j = 0; j < P; j++) {
      if (j == me) continue;
      if (p.S[j].len > 0) sends.push_back({j, (void*)(p.send + p.S[j].off), (size_t)p.S[j].len});
      if (p.R[j].len > 0) recvs.push_back({j, p.recv + p.R[j].off, (size_t)p.R[j].len});
    }
    CHK(c->tr->exchange(sends, recvs, k.s));
  }
  return k.end();
}

int moves_begin(mpjx_comm* c, int type, int* esz) {
  if (!c) return fail(MPJX_ERR_ARG, "comm is NULL");
  *esz = mpjx_type_size(type);
  if (*esz == 0) return fail(MPJX_ERR_ARG, "unknown datatype code %d", type);
  return MPJX_SUCCESS;
}

// ---- strided moves: mpjx_alltoallv_dt ------------------------------------------------------------------
// The general block move with a datatype per side (Contiguous / Vector, mpjx_strided_plan.hpp; Hvector /
// Indexed / Hindexed, mpjx_indexed_plan.hpp). Per rank, P send layouts and P receive layouts (SideBytes,
// absolute addresses); a segment moves the packed bytes of a send layout in order into the matching receive
// layout. A segment whose two layouts are contiguous runs k_moves, one whose two layouts are regular
// k_strided (mpjx_k_strided.hip) or, where it is an element transpose (plan_transpose_seg: a contiguous run
// against one granule per block with consecutive items on consecutive granules), k_transpose
// (mpjx_k_transpose.hip), every other one k_indexed (mpjx_k_indexed.hip), whose irregular sides read
// their type's device table from the launching communicator's cache (idx_table). "Strided" below means
// "not contiguous". The engines are moves_run's:
//   P = 1                     both types contiguous: the call IS mpjx_alltoallv's (byte ranges, moves_run);
//                             otherwise one k_strided or k_indexed launch
//   multicore, one device     share, rank 0 plans and launches the whole world's segments, fence. A
//                             base-type or packed-length mismatch between a sender and its receiver is
//                             MPJX_ERR_ARG on every rank before anything moves.
//   every other world         own block layout to layout; strided sends packed into scratch (one launch),
//                             the packed bytes through the transport's exchange, strided receives
//                             unpacked from scratch (one launch). A contiguous side is sent from, or
//                             received into, its buffer. Matching signatures are the caller's contract.

struct DtPlan {
  const char* send;
  char* recv;
  int base;  // the basic type code both types are made of
  std::vector<SideBytes> S, R;
};

int dt_check(mpjx_comm* c, const DtPlan& p) {
  int64_t st = 0, rt = 0;
  for (const SideBytes& x : p.S) st += x.total();
  for (const SideBytes& x : p.R) rt += x.total();
  if ((st > 0 && !p.send) || (rt > 0 && !p.recv)) return fail(MPJX_ERR_ARG, "NULL buffer with a nonzero count");
  CHK(check_bufs(c, st > 0 ? p.send : nullptr, rt > 0 ? p.recv : nullptr));
  int a = 0, b = 0;
  switch (strided_overlap(p.S, p.R, &a, &b)) {
    case kRecvOverlap: return fail(MPJX_ERR_ARG, "the receive layouts from ranks %d and %d overlap", a, b);
    case kSendRecvOverlap:
      return fail(MPJX_ERR_ARG, "the send layout to rank %d and the receive layout from rank %d overlap "
                  "(these collectives have no in-place form)", a, b);
    default: return MPJX_SUCCESS;  // none, or more blocks than the exact check expands: the caller's contract
  }
}

// The segments of one step of a call, by the kernel that runs them: one launch per kernel per table
struct DtMoves {
  MoveList ml;
  std::vector<StridedSeg> st;
  std::vector<IndexedSeg> ix;
  std::vector<TransposeSeg> tp;
  hipError_t launch(mpjx_comm* c, hipStream_t s) {
    c->move_kernels |= (ml.segs.empty() ? 0u : MPJX_MOVE_KERNEL_MOVES) | (st.empty() ? 0u : MPJX_MOVE_KERNEL_STRIDED) |
                       (ix.empty() ? 0u : MPJX_MOVE_KERNEL_INDEXED) | (tp.empty() ? 0u : MPJX_MOVE_KERNEL_TRANSPOSE);
    hipError_t e = launch_moves(ml, s);
    if (e == hipSuccess) e = launch_strided(st, s);
    if (e == hipSuccess) e = launch_transpose(tp, s);
    if (e == hipSuccess) e = launch_indexed(ix, s);
    return e;
  }
};

// MPJX_TRANSPOSE=0 (read per call, like MPJX_INDEXED_LDS_MAX_BLOCKS) sends every segment back to k_strided
bool transpose_on() {
  const char* e = getenv("MPJX_TRANSPOSE");
  return !(e && e[0] == '0' && e[1] == 0);
}

// The device table of an irregular layout, from c's cache: uploaded on `s` at first use. The cache entry
// keeps the host list alive, so the copy's source outlives it.
int idx_table(mpjx_comm* c, const SideBytes& x, hipStream_t s, const IdxEnt** out) {
  *out = nullptr;
  if (!x.irr) return MPJX_SUCCESS;
  auto it = c->idx_tables.find(x.code);
  if (it == c->idx_tables.end()) {
    void* dev = nullptr;
    const size_t bytes = x.irr->tab.size() * sizeof(IdxEnt);
    HIPCHK(hipMalloc(&dev, bytes));
    c->retired.push_back(dev);  // freed with the communicator
    HIPCHK(hipMemcpyAsync(dev, x.irr->tab.data(), bytes, hipMemcpyHostToDevice, s));
    it = c->idx_tables.emplace(x.code, mpjx_comm::IdxTable{(const IdxEnt*)dev, x.irr}).first;
  }
  *out = it->second.dev;
  return MPJX_SUCCESS;
}

// One segment onto the lists of the four kernels
int dt_add(mpjx_comm* c, hipStream_t st, const SideBytes& s, const SideBytes& d, DtMoves* m) {
  if (s.total() <= 0) return MPJX_SUCCESS;
  if (s.contiguous() && d.contiguous()) {
    m->ml.add((void*)(uintptr_t)d.base, (const void*)(uintptr_t)s.base, s.total());
    return MPJX_SUCCESS;
  }
  std::string err;
  if (s.regular() && d.regular()) {
    TransposeSeg ts;
    if (transpose_on() && plan_transpose_seg(s, d, &ts)) {
      m->tp.push_back(ts);
      return MPJX_SUCCESS;
    }
    StridedSeg sg;
    const int rc = plan_strided_seg(s, d, &sg, &err);
    if (rc != kTypeOk) return fail(rc, "%s", err.c_str());
    m->st.push_back(sg);
    return MPJX_SUCCESS;
  }
  const IdxEnt *stab, *dtab;
  CHK(idx_table(c, s, st, &stab));
  CHK(idx_table(c, d, st, &dtab));
  IndexedSeg sg;
  const int rc = plan_indexed_seg(s, stab, d, dtab, &sg, &err);
  if (rc != kTypeOk) return fail(rc, "%s", err.c_str());
  m->ix.push_back(sg);
  return MPJX_SUCCESS;
}

SideBytes packed_at(const char* p, int64_t bytes) {
  SideBytes x;
  x.base = (uint64_t)(uintptr_t)p;
  x.bb = x.sb = x.eb = bytes;
  x.nb = x.items = 1;
  return x;
}

int dt_run(mpjx_comm* c, DtPlan& p, void* stream) {
  c->move_kernels = 0;
  const int P = c->size, me = c->rank;
  auto* t = dynamic_cast<SmpTransport*>(c->tr.get());
  const bool world = P > 1 && t && smp_direct(c) && t->single();
  bool contig = true;
  for (int j = 0; j < P; j++) contig = contig && p.S[(size_t)j].contiguous() && p.R[(size_t)j].contiguous();
  if (P == 1 && contig) {  // exactly mpjx_alltoallv on the same bytes
    MovePlan m{p.send, p.recv, {}, {}};
    for (int j = 0; j < P; j++) {
      m.S.push_back(ByteRange{(int64_t)(p.S[(size_t)j].base - (uint64_t)(uintptr_t)p.send), p.S[(size_t)j].total()});
      m.R.push_back(ByteRange{(int64_t)(p.R[(size_t)j].base - (uint64_t)(uintptr_t)p.recv), p.R[(size_t)j].total()});
    }
    return moves_run(c, MV_ALLTOALL, m, p.base, stream);
  }
  CHK(dt_check(c, p));
  Call k;
  CHK(k.begin(c, stream, p.base));
  if (p.S[(size_t)me].total() != p.R[(size_t)me].total())
    return fail(MPJX_ERR_ARG, "rank %d sends itself %lld bytes but receives %lld", me,
                (long long)p.S[(size_t)me].total(), (long long)p.R[(size_t)me].total());
  DtMoves mv;
  if (world) {
    // The layouts stay in this rank's frame: no rank leaves the call before the fence's rendezvous
    std::vector<std::vector<const void*>> all;
    CHK(t->share(std::vector<const void*>{&p.S, &p.R, &p.base}, k.s, &all, true));
    auto S = [&](int i) -> const std::vector<SideBytes>& { return *(const std::vector<SideBytes>*)all[i][0]; };
    auto R = [&](int i) -> const std::vector<SideBytes>& { return *(const std::vector<SideBytes>*)all[i][1]; };
    for (int i = 0; i < P; i++)
      for (int j = 0; j < P; j++) {
        const long long sl = S(i)[(size_t)j].total(), rl = R(j)[(size_t)i].total();
        const int sb = *(const int*)all[i][2], rb = *(const int*)all[j][2];
        if (sl == rl && (sl == 0 || sb == rb)) continue;
        (void)t->fence(k.s, true);  // every rank has read every table before any rank returns
        if (sl != rl) return fail(MPJX_ERR_ARG, "rank %d sends %lld bytes to rank %d, which receives %lld", i, sl, j, rl);
        return fail(MPJX_ERR_ARG, "rank %d sends base type %d to rank %d, which receives base type %d", i, sb, j, rb);
      }
    if (me == 0) {
      for (int j = 0; j < P; j++)    // receiver
        for (int i = 0; i < P; i++)  // sender
          DCHK(dt_add(c, k.s, S(i)[(size_t)j], R(j)[(size_t)i], &mv));
      HIPCHK(mv.launch(c, k.s));
    }
    CHK(t->fence(k.s, true));
    return k.end();
  }
  CHK(dt_add(c, k.s, p.S[(size_t)me], p.R[(size_t)me], &mv));
  if (P == 1) {
    HIPCHK(mv.launch(c, k.s));
    return k.end();
  }
  // scratch slots (16-B aligned) of the strided sends, then of the strided receives
  std::vector<size_t> so((size_t)P, 0), ro((size_t)P, 0);
  size_t need = 0;
  auto slot = [&](const SideBytes& x, size_t* off) {
    if (x.total() <= 0 || x.contiguous()) return;
    *off = need;
    need += ((size_t)x.total() + 15) & ~(size_t)15;
  };
  for (int j = 0; j < P; j++)
    if (j != me) slot(p.S[(size_t)j], &so[(size_t)j]);
  for (int j = 0; j < P; j++)
    if (j != me) slot(p.R[(size_t)j], &ro[(size_t)j]);
  if (need) CHK(k.scratch(need));
  DtMoves unpack;
  std::vector<Xfer> sends, recvs;
  for (int j = 0; j < P; j++) {
    if (j == me) continue;
    const SideBytes& s = p.S[(size_t)j];
    const SideBytes& r = p.R[(size_t)j];
    if (s.total() > 0) {
      char* at = s.contiguous() ? (char*)(uintptr_t)s.base : c->scratch + so[(size_t)j];
      if (!s.contiguous()) CHK(dt_add(c, k.s, s, packed_at(at, s.total()), &mv));
      sends.push_back({j, at, (size_t)s.total()});
    }
    if (r.total() > 0) {
      char* at = r.contiguous() ? (char*)(uintptr_t)r.base : c->scratch + ro[(size_t)j];
      if (!r.contiguous()) CHK(dt_add(c, k.s, packed_at(at, r.total()), r, &unpack));
      recvs.push_back({j, at, (size_t)r.total()});
    }
  }
  HIPCHK(mv.launch(c, k.s));  // the own block and every peer's pack: one launch per kernel per table
  CHK(c->tr->exchange(sends, recvs, k.s));
  HIPCHK(unpack.launch(c, k.s));
  return k.end();
}

int dt_table(const TypeForm& f, const void* buf, const int64_t* counts, const int64_t* displs, int n,
             std::vector<SideBytes>* out, const char* what) {
  if (!counts || !displs) return fail(MPJX_ERR_ARG, "%s or their displacements are NULL", what);
  out->assign((size_t)n, SideBytes{});
  std::string err;
  for (int j = 0; j < n; j++)
    if (!plan_side(f, (uint64_t)(uintptr_t)buf, counts[j], displs[j], &(*out)[(size_t)j], &err, what))
      return fail(MPJX_ERR_ARG, "%s at index %d", err.c_str(), j);
  return MPJX_SUCCESS;
}

}  // namespace

static int alltoallv_dt_entry(mpjx_comm_t c, const void* sendbuf, const int64_t* sendcounts, const int64_t* sdispls,
                              int sendtype, void* recvbuf, const int64_t* recvcounts, const int64_t* rdispls,
                              int recvtype, void* stream) {
  if (!c) return fail(MPJX_ERR_ARG, "comm is NULL");
  TypeForm st, rt;
  if (!type_form(sendtype, &st)) return fail(MPJX_ERR_ARG, "unknown or freed datatype code %d", sendtype);
  if (!type_form(recvtype, &rt)) return fail(MPJX_ERR_ARG, "unknown or freed datatype code %d", recvtype);
  if (rt.irr && rt.irr->self_overlap)
    return fail(MPJX_ERR_ARG, "recvtype %d has blocks that share a byte: it can be sent, not received into", recvtype);
  if (st.base != rt.base)
    return fail(MPJX_ERR_ARG, "sendtype %d (base type %d) and recvtype %d (base type %d) differ in their base type",
                sendtype, st.base, recvtype, rt.base);
  DtPlan p{(const char*)sendbuf, (char*)recvbuf, st.base, {}, {}};
  CHK(dt_table(st, sendbuf, sendcounts, sdispls, c->size, &p.S, "sendcounts"));
  CHK(dt_table(rt, recvbuf, recvcounts, rdispls, c->size, &p.R, "recvcounts"));
  return dt_run(c, p, stream);
}

// ---- mpjx_pack / mpjx_unpack / mpjx_pack_size (Comm.Pack, Unpack, Pack_size: src/mpi/Comm.java:1860-1983) ----
// One mpjbuf section from, or into, `count` items of any datatype: the section arithmetic and the descriptor
// are mpjx_pack_plan.hpp's, the kernel k_pack (mpjx_k_pack.hip: layout, byte swap and header in one pass).
// Local calls: no rank waits for another, and a rejected call does not fail the world. Every argument is
// checked before the communicator is touched, so the checks need no device.
static int pack_entry(mpjx_comm_t c, bool unpack, const void* buf, int64_t count, int type, const void* image,
                      int64_t image_bytes, int64_t* position, int* status, void* stream) {
  const char* who = unpack ? "mpjx_unpack" : "mpjx_pack";
  TypeForm f;
  if (!type_form(type, &f)) return fail(MPJX_ERR_ARG, "%s: unknown or freed datatype code %d", who, type);
  if (!position) return fail(MPJX_ERR_ARG, "%s: position is NULL", who);
  PackSection sec;
  std::string err;
  if (!plan_pack_section(*position, count, f.size(), f.bsz, image_bytes, &sec, &err))
    return fail(MPJX_ERR_ARG, "%s: %s", who, err.c_str());
  if (!image) return fail(MPJX_ERR_ARG, "%s: image is NULL", who);
  if (unpack && !status) return fail(MPJX_ERR_ARG, "%s: status is NULL", who);
  if (sec.words > 0 && !buf)
    return fail(MPJX_ERR_ARG, "%s: NULL %s with count %lld", who, unpack ? "outbuf" : "inbuf", (long long)count);
  if (sec.words > 0 && (uintptr_t)buf % (uintptr_t)f.bsz)
    return fail(MPJX_ERR_ARG, "%s: %s %p is not aligned to the %d-byte base element", who, unpack ? "outbuf" : "inbuf",
                buf, f.bsz);
  if ((uintptr_t)image % 8)
    return fail(MPJX_ERR_ARG, "%s: image %p is not 8-byte aligned (the mpjbuf ALIGNMENT_UNIT)", who, image);
  if (unpack && f.irr && f.irr->self_overlap)
    return fail(MPJX_ERR_ARG, "%s: datatype %d has blocks that share a byte: it can be packed, not unpacked into", who,
                type);
  SideBytes lay;
  if (!plan_side(f, (uint64_t)(uintptr_t)buf, count, 0, &lay, &err)) return fail(MPJX_ERR_ARG, "%s: %s", who, err.c_str());
  if (unpack && lay.items_may_overlap()) {  // items closer together than their blocks reach (an explicit extent)
    int a = 0, b = 0;
    if (strided_overlap({}, {lay}, &a, &b) == kRecvOverlap)
      return fail(MPJX_ERR_ARG, "%s: %lld items of datatype %d (extent %lld) share a byte: they can be packed, not "
                  "unpacked into", who, (long long)count, type, (long long)f.extent());
  }
  if (!c) return fail(MPJX_ERR_ARG, "%s: comm is NULL", who);
  if (sec.words > 0) CHK(check_dev_ptr(buf, unpack ? "outbuf" : "inbuf"));
  CHK(check_dev_ptr(image, "image"));
  if (unpack) CHK(check_dev_ptr(status, "status"));
  Call k;
  CHK(k.begin(c, stream, f.base));
  const IdxEnt* tab = nullptr;
  if (sec.words > 0) CHK(idx_table(c, lay, k.s, &tab));
  PackSeg sg;
  plan_pack_seg(lay, tab, (uint64_t)(uintptr_t)image, image_bytes, sec, f.base, f.bsz, status, &sg);
  const hipError_t e = launch_pack(sg, unpack, k.s);
  if (e == hipErrorNoBinaryForGpu || e == hipErrorInvalidDeviceFunction)
    return fail(MPJX_ERR_NO_DEVICE, "no gfx950 kernel image for this device: %s", hipGetErrorString(e));
  if (e != hipSuccess) return fail(MPJX_ERR_HIP, "%s launch: %s", who, hipGetErrorString(e));
  *position = sec.end;
  return k.end();
}

extern "C" int mpjx_pack_size(int64_t count, int type, int64_t* bytes) {
  TypeForm f;
  if (!type_form(type, &f)) return fail(MPJX_ERR_ARG, "mpjx_pack_size: unknown or freed datatype code %d", type);
  if (!bytes) return fail(MPJX_ERR_ARG, "mpjx_pack_size: bytes is NULL");
  if (count < 0) return fail(MPJX_ERR_ARG, "mpjx_pack_size: negative count %lld", (long long)count);
  const int64_t item = f.size() * f.bsz;  // <= 2^62 (the type constructors)
  if (item > 0 && count > (kMoveMaxBytes - 16) / item)
    return fail(MPJX_ERR_ARG, "mpjx_pack_size: %lld items of %lld bytes reach beyond 2^62 bytes", (long long)count,
                (long long)item);
  *bytes = pack_size_bytes(count, item);
  return MPJX_SUCCESS;
}

extern "C" int mpjx_pack(mpjx_comm_t c, const void* inbuf, int64_t count, int type, void* image, int64_t image_bytes,
                         int64_t* position, void* stream) {
  return pack_entry(c, false, inbuf, count, type, image, image_bytes, position, nullptr, stream);
}

extern "C" int mpjx_unpack(mpjx_comm_t c, const void* image, int64_t image_bytes, int64_t* position, void* outbuf,
                           int64_t count, int type, int* status, void* stream) {
  return pack_entry(c, true, outbuf, count, type, image, image_bytes, position, status, stream);
}

static int allgather_entry(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, void* stream) {
  int esz;
  CHK(moves_begin(c, type, &esz));
  MovePlan p{(const char*)sendbuf, (char*)recvbuf, {}, {}};
  std::string err;
  if (!plan_equal(count, c->size, esz, &p.R, &err)) return plan_fail(err);
  CHK(plan_single(&p.S, c->size, -1, count, esz, "count"));
  return moves_run(c, MV_ALLGATHER, p, type, stream);
}

static int allgatherv_entry(mpjx_comm_t c, const void* sendbuf, int64_t sendcount, void* recvbuf,
                            const int64_t* recvcounts, const int64_t* displs, int type, void* stream) {
  int esz;
  CHK(moves_begin(c, type, &esz));
  MovePlan p{(const char*)sendbuf, (char*)recvbuf, {}, {}};
  CHK(plan_table(&p.R, c->size, recvcounts, displs, esz, "recvcounts"));
  CHK(plan_single(&p.S, c->size, -1, sendcount, esz, "sendcount"));
  return moves_run(c, MV_EXCHANGE, p, type, stream);
}

static int gatherv_entry(mpjx_comm_t c, const void* sendbuf, int64_t sendcount, void* recvbuf,
                         const int64_t* recvcounts, const int64_t* displs, int type, int root, void* stream) {
  int esz;
  CHK(moves_begin(c, type, &esz));
  CHK(check_root(c, root));
  MovePlan p{(const char*)sendbuf, (char*)recvbuf, {}, {}};
  if (c->rank == root) CHK(plan_table(&p.R, c->size, recvcounts, displs, esz, "recvcounts"));
  else p.R.assign((size_t)c->size, ByteRange{0, 0});
  CHK(plan_single(&p.S, c->size, root, sendcount, esz, "sendcount"));
  return moves_run(c, MV_EXCHANGE, p, type, stream);
}

static int scatterv_entry(mpjx_comm_t c, const void* sendbuf, const int64_t* sendcounts, const int64_t* displs,
                          void* recvbuf, int64_t recvcount, int type, int root, void* stream) {
  int esz;
  CHK(moves_begin(c, type, &esz));
  CHK(check_root(c, root));
  MovePlan p{(const char*)sendbuf, (char*)recvbuf, {}, {}};
  if (c->rank == root) CHK(plan_table(&p.S, c->size, sendcounts, displs, esz, "sendcounts"));
  else p.S.assign((size_t)c->size, ByteRange{0, 0});
  CHK(plan_single(&p.R, c->size, root, recvcount, esz, "recvcount"));
  return moves_run(c, MV_EXCHANGE, p, type, stream);
}

static int alltoall_entry(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, void* stream) {
  int esz;
  CHK(moves_begin(c, type, &esz));
  MovePlan p{(const char*)sendbuf, (char*)recvbuf, {}, {}};
  std::string err;
  if (!plan_equal(count, c->size, esz, &p.S, &err)) return plan_fail(err);
  p.R = p.S;
  return moves_run(c, MV_ALLTOALL, p, type, stream);
}

static int alltoallv_entry(mpjx_comm_t c, const void* sendbuf, const int64_t* sendcounts, const int64_t* sdispls,
                           void* recvbuf, const int64_t* recvcounts, const int64_t* rdispls, int type,
                           void* stream) {
  int esz;
  CHK(moves_begin(c, type, &esz));
  MovePlan p{(const char*)sendbuf, (char*)recvbuf, {}, {}};
  CHK(plan_table(&p.S, c->size, sendcounts, sdispls, esz, "sendcounts"));
  CHK(plan_table(&p.R, c->size, recvcounts, rdispls, esz, "recvcounts"));
  return moves_run(c, MV_ALLTOALL, p, type, stream);
}

// ---- reductions on derived datatypes: mpjx_{reduce,allreduce,reduce_scatter,scan}_dt -----------------------
// `count` items of ONE type are read from sendbuf and written to recvbuf (item k at k x extent, lb not
// subtracted: plan_side), reduced element-wise over the packed sequence of base elements (or pairs) in the
// combine order of the contiguous call on the packed vectors. A basic or pair code IS that contiguous call.
// A derived code takes one of three engines (mpjx_comm_last_dt_form):
//   P = 1                     move: the copy of send into recv through the layouts (dt_add: k_moves /
//                             k_strided / k_indexed); in place, nothing
//   multicore, one device,    direct: every rank publishes its call (share), rank 0 checks that the ranks
//   2 <= P <= 8, every type   agree and that no rank's layouts overlap, and launches k_pway_dt
//   of one form               (mpjx_kernels_dt.hpp) over the one layout all P + Q buffers share; every rank
//                             fences. One kernel and two rendezvous, like the contiguous direct engine. A
//                             base-type or packed-length mismatch, or a rank whose send and receive layouts
//                             overlap, is MPJX_ERR_ARG on every rank before anything moves. Ranks whose types
//                             have equal signatures but different forms leave together for the pack path.
//   every other world         pack: sendbuf packed into the communicator's staging region (dtstage) by the
//                             layout kernels, the contiguous entry point's body on the packed vectors (its
//                             windows, one-shot, pipeline and flags), the result unpacked into recvbuf. A
//                             contiguous layout skips both passes.
// The reference is not followed here: PureIntracomm.Reduce copies count * datatype.size CONTIGUOUS elements
// (PureIntracomm.java:1937-1938) and the typed workers combine [offset, count) contiguous base elements
// whatever the type (SumDouble.java:52), so it defines no result for a layout with gaps; these calls follow
// MPI, as the equal-count moves do.

namespace {

enum RdKind { RD_REDUCE, RD_ALLREDUCE, RD_RSCATTER, RD_SCAN };

// One rank's call; in a direct world the ranks read each other's (share), so it stays in the caller's frame
// until the fence
struct RdCall {
  int kind = RD_ALLREDUCE;
  const char* send = nullptr;
  char* recv = nullptr;
  int64_t items = 0;            // items read from send: count, or the sum of recvcounts
  int64_t mine = 0;             // items written to recv (0 where recv is not significant)
  const int64_t* rc = nullptr;  // Reduce_scatter: recvcounts, in items
  int op = 0, root = 0;
  unsigned flags = 0;
  TypeForm f;
  int eff = 0;      // the element type of the reduction: the base code, or 0x100 | base for a type made of pairs
  int64_t epi = 1;  // elements of `eff` per item
  SideBytes S, R;   // the layouts of `items` items at send and of `mine` items at recv (absolute addresses)
  int bad = MPJX_SUCCESS;  // this rank's own verdict (its layouts overlap), published to the world
  std::string badmsg;
};

// The contiguous entry point's body on (s, r): counts in elements of q.eff
int rd_inner(mpjx_comm* c, const RdCall& q, const void* s, void* r, unsigned flags, void* stream) {
  const int64_t n = q.items * q.epi;
  switch (q.kind) {
    case RD_REDUCE: return reduce_entry(c, s, r, n, q.eff, q.op, q.root, flags, stream);
    case RD_ALLREDUCE: return allreduce_entry(c, s, r, n, q.eff, q.op, flags, stream);
    case RD_SCAN: return scan_entry(c, s, r, n, q.eff, q.op, flags, stream);
    default: break;
  }
  if (!c) return fail(MPJX_ERR_ARG, "comm is NULL");
  if (!q.rc) return reject(c, fail(MPJX_ERR_ARG, "recvcounts is NULL"));
  std::vector<int64_t> rc((size_t)c->size);
  for (int j = 0; j < c->size; j++) rc[(size_t)j] = q.rc[j] * q.epi;
  return reduce_scatter_entry(c, s, r, rc.data(), q.eff, q.op, flags, stream);
}

int dt_stage(Call& k, size_t bytes) { return grow_device(k.c, &k.c->dtstage, &k.c->dtstage_bytes, bytes, k.s); }

// `x` moved so that its buffer position is `buf` instead of `from`
SideBytes rebased(const SideBytes& x, const void* from, const void* buf) {
  SideBytes y = x;
  y.base = x.base - (uint64_t)(uintptr_t)from + (uint64_t)(uintptr_t)buf;
  return y;
}

// One k_pway_dt launch over granules [q0, q0 + nq) of `a.lay`
int rd_launch(const RdCall& q, int kind, int P, const void* const* in, void* const* out, int nout, int root,
              PwayDtArgs a, bool vec, hipStream_t s) {
  for (int p = 0; p < P; p++) a.in[p] = in[p];
  for (int r = 0; r < nout; r++) a.out[r] = out[r];
  a.root = root;
  a.nrep = kind == K_SCAN ? 1 : nout;
  const hipError_t e = launch_op_dt(q.op, q.eff, kind, P, a, s, vec);
  if (e == hipErrorNoBinaryForGpu || e == hipErrorInvalidDeviceFunction)
    return fail(MPJX_ERR_NO_DEVICE, "no gfx950 kernel image for this device: %s", hipGetErrorString(e));
  if (e != hipSuccess)
    return fail(MPJX_ERR_HIP, "kernel launch (op %s, type %s on a derived layout, kind %d, P %d): %s", op_name(q.op),
                type_name(q.eff), kind, P, hipGetErrorString(e));
  return MPJX_SUCCESS;
}
// The MST tree rooted at `root` (two ranks: the root's operand, then the other's, as Combine::mst_o)
int rd_mst(const RdCall& q, int P, const void* const* in, int root, void* const* out, int nout, const PwayDtArgs& a,
           bool vec, hipStream_t s) {
  if (P > 2) return rd_launch(q, K_MST, P, in, out, nout, root, a, vec, s);
  const void* lst[2] = {in[root], in[1 - root]};
  return rd_launch(q, K_FOLD, 2, lst, out, nout, 0, a, vec, s);
}
// The FT order: in[first], then every other rank ascending (Combine::ft)
int rd_ft(const RdCall& q, int P, const void* const* in, int first, void* out, const PwayDtArgs& a, bool vec,
          hipStream_t s) {
  const void* lst[MAXP];
  int m = 0;
  lst[m++] = in[first];
  for (int i = 0; i < P; i++)
    if (i != first) lst[m++] = in[i];
  return rd_launch(q, K_FOLD, P, lst, &out, 1, 0, a, vec, s);
}

// Rank 0 of a direct world: the k_pway_dt launch or launches of the whole world's call. Every rank's type has
// rank 0's form and every rank's counts are rank 0's (checked by the caller), so rank 0's own layout, moved
// to base 0, is the layout of all P send and all receive buffers.
int rd_direct(Call& k, const RdCall& q, const std::vector<const RdCall*>& all) {
  mpjx_comm* c = k.c;
  const int P = c->size;
  const SideBytes L = rebased(q.S, q.send, nullptr);
  if (L.total() <= 0) return MPJX_SUCCESS;
  const bool old = (q.flags & MPJX_FLAG_OLD_COLLECTIVES) != 0;
  const int64_t size_b = q.f.size() * q.f.bsz, ext_b = q.f.extent() * q.f.bsz;
  const void* in[MAXP];
  void* out[MAXP];
  std::vector<uint64_t> ptrs;
  int64_t item0 = 0;
  for (int j = 0; j < P; j++) {
    in[j] = all[(size_t)j]->send;
    out[j] = all[(size_t)j]->mine > 0 ? all[(size_t)j]->recv : nullptr;
    // Reduce_scatter: rank j's pointer moved back so that item item0 lands on its receive buffer's origin
    if (q.kind == RD_RSCATTER && out[j]) out[j] = (char*)out[j] - item0 * ext_b;
    if (q.kind == RD_RSCATTER) item0 += q.rc[j];
    ptrs.push_back((uint64_t)(uintptr_t)in[j]);
    if (out[j]) ptrs.push_back((uint64_t)(uintptr_t)out[j]);
  }
  const int esz = reduce_dt_elem_bytes(q.f);
  const uint32_t glog = reduce_dt_granule_log(L, esz, ptrs.data(), (int)ptrs.size());
  const IdxEnt* tab = nullptr;
  CHK(idx_table(c, q.S, k.s, &tab));
  PwayDtArgs a{};
  int64_t ngran = 0;
  std::string err;
  const int prc = plan_reduce_dt(L, glog, tab, &a.lay, &ngran, &err);
  if (prc != kTypeOk) return fail(prc, "%s", err.c_str());
  a.nq = (uint32_t)ngran;
  const bool vec = glog == 4;
  switch (q.kind) {
    case RD_REDUCE:
      return old ? rd_ft(q, P, in, q.root, out[q.root], a, vec, k.s)
                 : rd_mst(q, P, in, q.root, &out[q.root], 1, a, vec, k.s);
    case RD_SCAN: return rd_launch(q, K_SCAN, P, in, out, P, 0, a, vec, k.s);
    case RD_RSCATTER: {
      item0 = 0;
      for (int r = 0; r < P; item0 += q.rc[r], r++) {
        if (q.rc[r] <= 0) continue;
        const DtRange g = reduce_dt_range(item0, q.rc[r], size_b, ext_b, glog);
        a.q0 = g.q0;
        a.nq = g.nq;
        if (old) {  // FT_Reduce_scatter: x_0 folded with x_1 .. x_{P-1}
          CHK(rd_launch(q, K_FOLD, P, in, &out[r], 1, 0, a, vec, k.s));
        } else if (P <= 2 && !q.f.pair) {  // the BKT ring at P = 2: own block, then the successor's
          const void* lst[2] = {in[r], in[(r + 1) % P]};
          CHK(rd_launch(q, K_FOLD, 2, lst, &out[r], 1, 0, a, vec, k.s));
        } else {
          CHK(rd_mst(q, P, in, 0, &out[r], 1, a, vec, k.s));
        }
      }
      return MPJX_SUCCESS;
    }
    default: break;
  }
  if (!old) return rd_mst(q, P, in, 0, out, P, a, vec, k.s);  // MST(0) -> every rank's recv, one launch
  // FT_Allreduce: rank r's own fold order for rank r's recv. An in-place rank's recv is an input of every
  // later fold, so the results go through temporaries (the layout's span each) until all folds are done.
  bool alias = false;
  for (int j = 0; j < P; j++) alias = alias || in[j] == out[j];
  void* res[MAXP];
  for (int r = 0; r < P; r++) res[r] = out[r];
  if (alias) {
    uint64_t lo, hi;
    L.span(&lo, &hi);
    const size_t slot = round_up((size_t)(hi - lo) + 16, kAlignBytes);
    CHK(dt_stage(k, (size_t)P * slot));
    // 16-B aligned, like every granule's offset where the 16-B form was chosen
    for (int r = 0; r < P; r++) res[r] = c->dtstage + (size_t)r * slot + (lo & 15u) - lo;
  }
  for (int r = 0; r < P; r++) CHK(rd_ft(q, P, in, r, res[r], a, vec, k.s));
  if (alias) {
    DtMoves mv;
    for (int r = 0; r < P; r++) CHK(dt_add(c, k.s, rebased(q.S, q.send, res[r]), rebased(q.S, q.send, out[r]), &mv));
    HIPCHK(mv.launch(c, k.s));
  }
  return MPJX_SUCCESS;
}

int rd_run(mpjx_comm* c, RdCall& q, int type, void* stream) {
  if (!type_form(type, &q.f)) return fail(MPJX_ERR_ARG, "unknown or freed datatype code %d", type);
  if (type < kDerivedBase) {  // a basic or pair code: the contiguous call itself
    q.eff = type;
    q.epi = 1;
    if (c) c->dt_form = MPJX_DT_FORM_CONTIGUOUS;
    return rd_inner(c, q, q.send, q.recv, q.flags, stream);
  }
  q.eff = q.f.pair ? (0x100 | q.f.base) : q.f.base;
  q.epi = q.f.size() / (q.f.pair ? 2 : 1);
  {
    const int orc = mpjx_op_check(q.op, q.eff);
    if (orc != MPJX_SUCCESS) return reject(c, orc);
  }
  if (q.flags & MPJX_FLAG_FAITHFUL)
    return reject(c, fail(MPJX_ERR_UNSUPPORTED, "MPJX_FLAG_FAITHFUL with the derived datatype %d: the reference "
                                                "defines no result for a reduction on a layout", type));
  if (q.flags & (MPJX_FLAG_SEND_BIG_ENDIAN | MPJX_FLAG_RECV_BIG_ENDIAN))
    return reject(c, fail(MPJX_ERR_UNSUPPORTED, "big-endian buffers (flags 0x%x) with the derived datatype %d",
                          q.flags, type));
  if (q.f.irr && q.f.irr->self_overlap)
    return reject(c, fail(MPJX_ERR_ARG, "datatype %d has blocks that share a byte: a reduction receives into it", type));
  if (!c) return fail(MPJX_ERR_ARG, "comm is NULL");
  c->move_kernels = 0;
  const int P = c->size, me = c->rank;
  const int64_t count = q.mine;  // as passed (Reduce_scatter: unused)
  if (q.kind == RD_REDUCE) CHK(check_root(c, q.root));
  if (q.kind == RD_RSCATTER) {
    if (!q.rc) return reject(c, fail(MPJX_ERR_ARG, "recvcounts is NULL"));
    q.items = 0;
    for (int j = 0; j < P; j++) {
      if (q.rc[j] < 0) return reject(c, fail(MPJX_ERR_ARG, "recvcounts[%d] = %lld is negative", j, (long long)q.rc[j]));
      q.items += q.rc[j];
    }
    q.mine = q.rc[me];
  } else {
    if (count < 0) return reject(c, fail(MPJX_ERR_ARG, "negative count %lld", (long long)count));
    q.items = count;
    q.mine = (q.kind == RD_REDUCE && me != q.root) ? 0 : count;
  }
  std::string err;
  if (!plan_side(q.f, (uint64_t)(uintptr_t)q.send, q.items, 0, &q.S, &err, "count") ||
      !plan_side(q.f, (uint64_t)(uintptr_t)q.recv, q.mine, 0, &q.R, &err, "count"))
    return reject(c, fail(MPJX_ERR_ARG, "%s (datatype %d)", err.c_str(), type));
  const int64_t sb = q.S.total(), rb = q.R.total();
  if (rb == 0) q.mine = 0;
  if ((sb > 0 && !q.send) || (rb > 0 && !q.recv))
    return reject(c, fail(MPJX_ERR_ARG, "NULL buffer with %lld items of datatype %d", (long long)q.items, type));
  CHK(check_bufs(c, sb > 0 ? q.send : nullptr, rb > 0 ? q.recv : nullptr));
  // exactly in place (the same position, so the same layout on both sides) is the one overlap allowed;
  // Reduce_scatter's two layouts differ beyond one rank, so there it has no in-place form
  if (sb > 0 && rb > 0 && !((q.kind != RD_RSCATTER || P == 1) && (const char*)q.recv == q.send)) {
    int a = 0, b = 0;
    if (strided_overlap({q.S}, {q.R}, &a, &b) == kSendRecvOverlap) {
      q.bad = MPJX_ERR_ARG;
      char msg[256];
      snprintf(msg, sizeof msg, "rank %d: the layouts of datatype %d at sendbuf %p and at recvbuf %p share a byte "
               "(only sendbuf == recvbuf is in place%s)", me, type, (const void*)q.send, (void*)q.recv,
               q.kind == RD_RSCATTER ? "; Reduce_scatter has no in-place form" : "");
      q.badmsg = msg;
    }
  }
  // items closer together than their blocks reach (an explicit extent): the receive layout may overlap itself
  if (rb > 0 && !q.bad && q.R.items_may_overlap()) {
    int a = 0, b = 0;
    if (strided_overlap({}, {q.R}, &a, &b) == kRecvOverlap) {
      q.bad = MPJX_ERR_ARG;
      char msg[256];
      snprintf(msg, sizeof msg, "rank %d: %lld items of datatype %d (extent %lld) share a byte: a reduction receives "
               "into them", me, (long long)q.mine, type, (long long)q.f.extent());
      q.badmsg = msg;
    }
  }
  const bool blocking = (q.flags & MPJX_FLAG_BLOCKING) != 0;
  Call k;
  if (P == 1) {
    c->dt_form = MPJX_DT_FORM_MOVE;
    if (q.bad) return fail(q.bad, "%s", q.badmsg.c_str());
    CHK(k.begin(c, stream, q.eff));
    k.blocking = blocking;
    if (rb > 0 && (const char*)q.recv != q.send) {
      DtMoves mv;
      CHK(dt_add(c, k.s, q.S, q.R, &mv));
      HIPCHK(mv.launch(c, k.s));
    }
    CHK(k.end());
    return finish_blocking(c, q.flags, stream);
  }
  auto* t = dynamic_cast<SmpTransport*>(c->tr.get());
  if (P <= MAXP && t && smp_direct(c) && t->single()) {
    CHK(k.begin(c, stream, q.eff));
    k.blocking = blocking;
    std::vector<std::vector<const void*>> shared;
    CHK(t->share(std::vector<const void*>{&q}, k.s, &shared, true));
    std::vector<const RdCall*> all((size_t)P);
    for (int j = 0; j < P; j++) all[(size_t)j] = (const RdCall*)shared[(size_t)j][0];
    // every rank reads every rank's call and reaches the same verdict
    int bad = MPJX_SUCCESS;
    char msg[384] = "";
    bool same = true;
    for (int j = 0; j < P && !bad; j++) {
      const RdCall& x = *all[(size_t)j];
      const RdCall& z = *all[0];
      if (x.bad) {
        bad = x.bad;
        snprintf(msg, sizeof msg, "%s", x.badmsg.c_str());
      } else if (x.eff != z.eff) {
        bad = MPJX_ERR_ARG;
        snprintf(msg, sizeof msg, "rank %d reduces base type %s but rank 0 base type %s", j, type_name(x.eff), type_name(z.eff));
      } else if (x.items * x.epi != z.items * z.epi) {
        bad = MPJX_ERR_ARG;
        snprintf(msg, sizeof msg, "rank %d reduces %lld elements but rank 0 reduces %lld", j, (long long)(x.items * x.epi),
                 (long long)(z.items * z.epi));
      } else if (x.kind != z.kind || x.op != z.op || (x.kind == RD_REDUCE && x.root != z.root) ||
                 ((x.flags ^ z.flags) & MPJX_FLAG_OLD_COLLECTIVES)) {
        bad = MPJX_ERR_ARG;
        snprintf(msg, sizeof msg, "rank %d and rank 0 differ in the collective, its op, root or flags", j);
      }
      for (int r = 0; r < P && !bad && x.kind == RD_RSCATTER; r++)
        if (x.rc[r] * x.epi != z.rc[r] * z.epi) {
          bad = MPJX_ERR_ARG;
          snprintf(msg, sizeof msg, "rank %d gives rank %d %lld elements but rank 0 gives it %lld", j, r,
                   (long long)(x.rc[r] * x.epi), (long long)(z.rc[r] * z.epi));
        }
      same = same && x.items == z.items && same_form(x.f, z.f);
    }
    if (bad || !same) {
      (void)t->fence(k.s, true);  // every rank has read every call before any rank's frame goes
      if (bad) return fail(bad, "%s", msg);
      CHK(k.end());
    } else {
      c->dt_form = MPJX_DT_FORM_DIRECT;
      if (me == 0) DCHK(rd_direct(k, q, all));
      CHK(t->fence(k.s, true, false, blocking));
      CHK(k.end());
      return finish_blocking(c, q.flags, stream);
    }
  } else if (q.bad) {
    return reject(c, fail(q.bad, "%s", q.badmsg.c_str()));
  }
  // the pack path
  c->dt_form = MPJX_DT_FORM_PACK;
  CHK(k.begin(c, stream, q.eff));
  const bool pack = sb > 0 && !q.S.contiguous(), unpack = rb > 0 && !q.R.contiguous();
  const size_t shalf = pack ? round_up((size_t)sb, kAlignBytes) : 0;
  if (pack || unpack) CHK(dt_stage(k, shalf + (unpack ? round_up((size_t)rb, kAlignBytes) : 0)));
  const char* ps = pack ? c->dtstage : sb > 0 ? (const char*)(uintptr_t)q.S.base : q.send;
  char* pr = unpack ? c->dtstage + shalf : rb > 0 ? (char*)(uintptr_t)q.R.base : nullptr;
  if (pack) {
    DtMoves mv;
    CHK(dt_add(c, k.s, q.S, packed_at(ps, sb), &mv));
    HIPCHK(mv.launch(c, k.s));
  }
  CHK(k.end());
  CHK(rd_inner(c, q, ps, pr, q.flags & ~MPJX_FLAG_BLOCKING, k.s));
  if (unpack) {
    DtMoves mv;
    CHK(dt_add(c, k.s, packed_at(pr, rb), q.R, &mv));
    HIPCHK(mv.launch(c, k.s));
  }
  CHK(k.end());
  return finish_blocking(c, q.flags, stream);
}

int rd_call(mpjx_comm* c, int kind, const void* sendbuf, void* recvbuf, int64_t count, const int64_t* recvcounts,
            int type, int op, int root, unsigned flags, void* stream) {
  RdCall q;
  q.kind = kind;
  q.send = (const char*)sendbuf;
  q.recv = (char*)recvbuf;
  q.items = q.mine = count;
  q.rc = recvcounts;
  q.op = op;
  q.root = root;
  q.flags = flags;
  return rd_run(c, q, type, stream);
}

}  // namespace

// The C-ABI entry points. A call that fails leaves this rank out of step with its peers (it skipped the
// collective, or stopped between two of its transport steps): `ended` tells the transport
// (Transport::call_failed). Multicore and IPC worlds are marked failed, so peers waiting for this rank
// — a failed scratch allocation before the first rendezvous, say — error out instead of waiting
// forever; at P > 1 an RCCL communicator is aborted, so the rank's next call fails instead of pairing
// with the peers' pending exchange (include/mpjx.h).
static int ended(mpjx_comm* c, int rc) {
  if (rc != MPJX_SUCCESS && c && c->tr) c->tr->call_failed();
  return rc;
}

extern "C" int mpjx_bcast(mpjx_comm_t c, void* buf, int64_t count, int type, int root, void* stream) {
  return ended(c, bcast_entry(c, buf, count, type, root, stream));
}

extern "C" int mpjx_gather(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, int root,
                           void* stream) {
  return ended(c, gather_entry(c, sendbuf, recvbuf, count, type, root, stream));
}

extern "C" int mpjx_scatter(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, int root,
                            void* stream) {
  return ended(c, scatter_entry(c, sendbuf, recvbuf, count, type, root, stream));
}

extern "C" int mpjx_allgather(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type,
                              void* stream) {
  return ended(c, allgather_entry(c, sendbuf, recvbuf, count, type, stream));
}

extern "C" int mpjx_allgatherv(mpjx_comm_t c, const void* sendbuf, int64_t sendcount, void* recvbuf,
                               const int64_t* recvcounts, const int64_t* displs, int type, void* stream) {
  return ended(c, allgatherv_entry(c, sendbuf, sendcount, recvbuf, recvcounts, displs, type, stream));
}

extern "C" int mpjx_gatherv(mpjx_comm_t c, const void* sendbuf, int64_t sendcount, void* recvbuf,
                            const int64_t* recvcounts, const int64_t* displs, int type, int root, void* stream) {
  return ended(c, gatherv_entry(c, sendbuf, sendcount, recvbuf, recvcounts, displs, type, root, stream));
}

extern "C" int mpjx_scatterv(mpjx_comm_t c, const void* sendbuf, const int64_t* sendcounts, const int64_t* displs,
                             void* recvbuf, int64_t recvcount, int type, int root, void* stream) {
  return ended(c, scatterv_entry(c, sendbuf, sendcounts, displs, recvbuf, recvcount, type, root, stream));
}

extern "C" int mpjx_alltoall(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type,
                             void* stream) {
  return ended(c, alltoall_entry(c, sendbuf, recvbuf, count, type, stream));
}

extern "C" int mpjx_alltoallv(mpjx_comm_t c, const void* sendbuf, const int64_t* sendcounts, const int64_t* sdispls,
                              void* recvbuf, const int64_t* recvcounts, const int64_t* rdispls, int type,
                              void* stream) {
  return ended(c, alltoallv_entry(c, sendbuf, sendcounts, sdispls, recvbuf, recvcounts, rdispls, type, stream));
}

extern "C" int mpjx_alltoallv_dt(mpjx_comm_t c, const void* sendbuf, const int64_t* sendcounts,
                                 const int64_t* sdispls, int sendtype, void* recvbuf, const int64_t* recvcounts,
                                 const int64_t* rdispls, int recvtype, void* stream) {
  return ended(c, alltoallv_dt_entry(c, sendbuf, sendcounts, sdispls, sendtype, recvbuf, recvcounts, rdispls, recvtype,
                                     stream));
}

extern "C" int mpjx_allreduce(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, int op,
                              unsigned flags, void* stream) {
  return ended(c, allreduce_entry(c, sendbuf, recvbuf, count, type, op, flags, stream));
}

extern "C" int mpjx_reduce(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, int op,
                           int root, unsigned flags, void* stream) {
  return ended(c, reduce_entry(c, sendbuf, recvbuf, count, type, op, root, flags, stream));
}

extern "C" int mpjx_reduce_scatter(mpjx_comm_t c, const void* sendbuf, void* recvbuf, const int64_t* recvcounts,
                                   int type, int op, unsigned flags, void* stream) {
  return ended(c, reduce_scatter_entry(c, sendbuf, recvbuf, recvcounts, type, op, flags, stream));
}

extern "C" int mpjx_scan(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, int op,
                         unsigned flags, void* stream) {
  return ended(c, scan_entry(c, sendbuf, recvbuf, count, type, op, flags, stream));
}

extern "C" int mpjx_reduce_dt(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, int op,
                              int root, unsigned flags, void* stream) {
  return ended(c, rd_call(c, RD_REDUCE, sendbuf, recvbuf, count, nullptr, type, op, root, flags, stream));
}

extern "C" int mpjx_allreduce_dt(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, int op,
                                 unsigned flags, void* stream) {
  return ended(c, rd_call(c, RD_ALLREDUCE, sendbuf, recvbuf, count, nullptr, type, op, 0, flags, stream));
}

extern "C" int mpjx_reduce_scatter_dt(mpjx_comm_t c, const void* sendbuf, void* recvbuf, const int64_t* recvcounts,
                                      int type, int op, unsigned flags, void* stream) {
  return ended(c, rd_call(c, RD_RSCATTER, sendbuf, recvbuf, 0, recvcounts, type, op, 0, flags, stream));
}

extern "C" int mpjx_scan_dt(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, int op,
                            unsigned flags, void* stream) {
  return ended(c, rd_call(c, RD_SCAN, sendbuf, recvbuf, count, nullptr, type, op, 0, flags, stream));
}

extern "C" int mpjx_comm_last_move_kernels(mpjx_comm_t c, unsigned* mask) {
  COMM_ARG(c);
  if (!mask) return fail(MPJX_ERR_ARG, "NULL argument");
  *mask = c->move_kernels;
  return MPJX_SUCCESS;
}

extern "C" int mpjx_comm_last_dt_form(mpjx_comm_t c, int* form) {
  COMM_ARG(c);
  if (!form) return fail(MPJX_ERR_ARG, "NULL argument");
  *form = c->dt_form;
  return MPJX_SUCCESS;
}

extern "C" int mpjx_allreduce_host(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, int op,
                                   unsigned flags) {
  return ended(c, allreduce_host_entry(c, sendbuf, recvbuf, count, type, op, flags));
}

extern "C" int mpjx_reduce_host(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, int op,
                                int root, unsigned flags) {
  return ended(c, reduce_host_entry(c, sendbuf, recvbuf, count, type, op, root, flags));
}

extern "C" int mpjx_scan_host(mpjx_comm_t c, const void* sendbuf, void* recvbuf, int64_t count, int type, int op,
                              unsigned flags) {
  return ended(c, scan_host_entry(c, sendbuf, recvbuf, count, type, op, flags));
}

extern "C" int mpjx_reduce_scatter_host(mpjx_comm_t c, const void* sendbuf, void* recvbuf, const int64_t* recvcounts,
                                        int type, int op, unsigned flags) {
  return ended(c, reduce_scatter_host_entry(c, sendbuf, recvbuf, recvcounts, type, op, flags));
}

// ---- what the point-to-point calls (mpjx_p2p.hip) share with the block moves -------------------------------------
namespace mpjx {

int p2p_idx_table(mpjx_comm* c, const SideBytes& x, hipStream_t s, const IdxEnt** out) { return idx_table(c, x, s, out); }

bool p2p_transpose_on() { return transpose_on(); }

// MPJX_P2P_BATCH=0: the batch through DtMoves::launch, one launch per kernel family per table, for comparison
// with k_msgs. A message shorter than its receive layout never takes k_transpose, which walks the whole of X.
int p2p_launch_families(mpjx_comm* c, hipStream_t s, const std::vector<std::pair<SideBytes, SideBytes>>& msgs) {
  DtMoves mv;
  std::string err;
  for (const auto& m : msgs) {
    const SideBytes &a = m.first, &b = m.second;
    if (a.total() <= 0) continue;
    if (a.contiguous() && b.contiguous()) {
      mv.ml.add((void*)(uintptr_t)b.base, (const void*)(uintptr_t)a.base, a.total());
    } else if (a.regular() && b.regular()) {
      TransposeSeg ts;
      StridedSeg sg;
      if (a.total() == b.total() && transpose_on() && plan_transpose_seg(a, b, &ts)) {
        mv.tp.push_back(ts);
        continue;
      }
      const int rc = plan_strided_seg(a, b, &sg, &err);
      if (rc != kTypeOk) return fail(rc, "%s", err.c_str());
      mv.st.push_back(sg);
    } else {
      const IdxEnt *stab, *dtab;
      CHK(idx_table(c, a, s, &stab));
      CHK(idx_table(c, b, s, &dtab));
      IndexedSeg sg;
      const int rc = plan_indexed_seg(a, stab, b, dtab, &sg, &err);
      if (rc != kTypeOk) return fail(rc, "%s", err.c_str());
      mv.ix.push_back(sg);
    }
  }
  c->move_kernels = 0;
  HIPCHK(mv.launch(c, s));
  return MPJX_SUCCESS;
}

}  // namespace mpjx
