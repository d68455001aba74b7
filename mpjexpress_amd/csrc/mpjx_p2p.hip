// mpjx_p2p.hip — the point-to-point calls of libmpjx on device buffers: Send, Recv, Isend, Irecv, Sendrecv,
// Sendrecv_replace, Wait, Test, Waitall (src/mpi/Comm.java:381, :882, :1446, :1578, :2301, :2392;
// src/mpi/Request.java:81, :159; src/mpi/Status.java:81, :173), exported through the C ABI of include/mpjx.h.
//
// Matching is the Mailbox's (mpjx_p2p_plan.hpp, one per multicore world, apart from the collectives' barrier).
// This file posts requests, and moves matched pairs:
//   post      the layout of `count` items of the type (plan_side), the argument checks, a ready event on the
//             communicator's stream unless it is idle (as SmpTransport::share), Mailbox::post. No launch.
//   progress  every call that waits claims EVERY matched pair its rank is a party to, makes its stream wait on
//             the peers' ready events, moves the batch — k_msgs (mpjx_k_msgs.hip), one launch per kMsgsMax
//             messages of any layout kinds; element transposes through launch_transpose — records one
//             completion event for the batch and marks the pairs LAUNCHED. The other party's wait orders its
//             stream after that event. MPJX_P2P_BATCH=0 sends the batch through DtMoves::launch instead.
//   wait      sleeps on the mailbox's condition variable while a request is unmatched (nothing is enqueued on
//             the GPU for it), bounded by MPJX_P2P_TIMEOUT_S / mpjx_comm_set_p2p_timeout and by the world's
//             `failed` flag; ends with Transport::wait on the stream, as MPJX_FLAG_BLOCKING does.
//   persistent  Send_init / Recv_init keep the checked request of plan_req (Persist, mpjx_p2p_plan.hpp); Start and
//             Startall post a fresh copy of it (Startall: one stream query, one ready event, one lock acquisition
//             for the whole list). A pair of two persistent requests has the same segment at every start: after
//             its first move the segment is stored in the communicator's device pool (mpjx_msgs_pool_plan.hpp),
//             and a batch ALL of whose pairs are pooled goes out through k_msgs_pool (mpjx_k_msgs_pool.hip), one
//             launch per kPoolBatchMax pairs. MPJX_P2P_POOL=0 keeps every batch on the path above.
//   wire      MPI.PACKED (base 9, an mpjbuf image counted in bytes) is taken by the eight calls that post. A pair
//             with PACKED on exactly one side is packed or unpacked on the fly by k_wire (mpjx_k_wire.hip), one
//             launch per kWireMax such pairs of a batch, beside the k_msgs launch for the rest; an unpack's header
//             is checked on the device and its outcome {code, n} comes back through a pinned 8-byte slot that the
//             first wait to see the batch complete reads (resolve_wire). Probe / Iprobe peek at the mailbox.
// Supported worlds: multicore worlds whose ranks address each other's memory (SmpWorld::direct), P = 1
// included. The several-device form has no machine to be run on and is unverified.
#include "mpjx_internal.hpp"

#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <utility>

using namespace mpjx;

namespace mpjx {
int p2p_idx_table(mpjx_comm* c, const SideBytes& x, hipStream_t s, const IdxEnt** out);
bool p2p_transpose_on();
int p2p_launch_families(mpjx_comm* c, hipStream_t s, const std::vector<std::pair<SideBytes, SideBytes>>& msgs);
}  // namespace mpjx

struct mpjx_request {
  std::shared_ptr<P2PReq> q;                   // the posted request of a plain handle (req_of)
  std::shared_ptr<Persist> pr;                 // a persistent request (mpjx_send_init / mpjx_recv_init): q stays empty
  mpjx_comm* c = nullptr;
  std::shared_ptr<SmpWorld> w;                 // keeps the mailbox and the world's `failed` flag alive
  std::shared_ptr<std::atomic<bool>> alive;    // false once the communicator is destroyed: c dangles
};

namespace {

struct Ev {
  hipEvent_t e = nullptr;
  ~Ev() {
    if (e) (void)hipEventDestroy(e);
  }
};

int record_event(hipStream_t s, std::shared_ptr<void>* out) {
  auto ev = std::make_shared<Ev>();
  HIPCHK(hipEventCreateWithFlags(&ev->e, hipEventDisableTiming));
  HIPCHK(hipEventRecord(ev->e, s));
  *out = ev;
  return MPJX_SUCCESS;
}
hipEvent_t event_of(const std::shared_ptr<void>& p) { return p ? static_cast<Ev*>(p.get())->e : nullptr; }

double env_double(const char* name, double dflt) {
  const char* e = getenv(name);
  const double v = e ? atof(e) : 0;
  return v > 0 ? v : dflt;
}

// The world of a point-to-point call: MPJX_ERR_UNSUPPORTED outside direct multicore worlds
int p2p_world(mpjx_comm* c, SmpTransport** out, bool usable = true) {
  COMM_ARG(c);
  auto* t = dynamic_cast<SmpTransport*>(c->tr.get());
  if (!t || !t->w->direct || !t->w->mail)
    return fail(MPJX_ERR_UNSUPPORTED, "point-to-point calls are provided for multicore worlds whose ranks address each "
                "other's memory, not for the %s engine", c->tr ? c->tr->name() : "?");
  if (usable && t->w->failed.load(std::memory_order_acquire))
    return fail(MPJX_ERR_INTERNAL, "multicore world: another rank failed; the communicator is unusable");
  *out = t;
  return MPJX_SUCCESS;
}

// The stream of the call, ordered after the previous call's (Call::begin of the collectives)
int p2p_begin(mpjx_comm* c, hipStream_t* s) {
  HIPCHK(hipSetDevice(c->device));
  *s = c->stream;
  if (c->last_stream && c->last_stream != *s) {
    if (!c->last_recorded) HIPCHK(hipEventRecord(c->last_ev, c->last_stream));
    HIPCHK(hipStreamWaitEvent(*s, c->last_ev, 0));
  }
  c->last_stream = *s;
  c->last_recorded = false;
  return MPJX_SUCCESS;
}

// The checks before posting and the request of `count` items of `type` at buf. Nothing is posted.
int plan_req(mpjx_comm* c, bool send, const void* buf, int64_t count, int type, int peer, int tag,
             std::shared_ptr<P2PReq>* out) {
  const char* who = send ? "send" : "receive";
  TypeForm f;
  // MPI.PACKED: buf is an mpjbuf image, count its length (send) or room (receive) in bytes: a run of 1-byte words
  const bool packed = type == MPJX_PACKED;
  if (!(packed ? basic_form(MPJX_BYTE, &f) : type_form(type, &f)))
    return fail(MPJX_ERR_ARG, "%s: unknown or freed datatype code %d", who, type);
  if (count < 0) return fail(MPJX_ERR_ARG, "%s: negative count %lld", who, (long long)count);
  if (packed && (uintptr_t)buf % 8)
    return fail(MPJX_ERR_ARG, "%s: image %p is not 8-byte aligned (the mpjbuf ALIGNMENT_UNIT)", who, buf);
  const bool wild = !send && peer == MPJX_ANY_SOURCE;
  if (!(peer >= 0 && peer < c->size) && peer != MPJX_PROC_NULL && !wild)
    return fail(MPJX_ERR_ARG, "%s: rank %d out of range (the communicator has %d)", who, peer, c->size);
  if (tag < 0 && !(!send && tag == MPJX_ANY_TAG)) return fail(MPJX_ERR_ARG, "%s: tag %d is negative", who, tag);
  if (!send && f.irr && f.irr->self_overlap)
    return fail(MPJX_ERR_ARG, "receive: datatype %d has blocks that share a byte: it can be sent, not received into", type);
  auto q = std::make_shared<P2PReq>();
  std::string err;
  if (!plan_side(f, (uint64_t)(uintptr_t)buf, count, 0, &q->lay, &err)) return fail(MPJX_ERR_ARG, "%s: %s", who, err.c_str());
  q->send = send;
  q->rank = c->rank;
  q->peer = peer;
  q->tag = tag;
  q->base = packed ? kP2PPacked : f.base;
  q->bsz = f.bsz;
  q->bytes = q->lay.total();
  q->count = count;
  q->empty_type = f.size() == 0;
  if (q->bytes > 0 && !buf) return fail(MPJX_ERR_ARG, "%s: NULL buffer with count %lld", who, (long long)count);
  if (q->bytes > 0 && peer != MPJX_PROC_NULL) CHK(check_dev_ptr(buf, "buffer"));
  if (!send && q->lay.items_may_overlap()) {
    int a = 0, b = 0;
    if (strided_overlap({}, {q->lay}, &a, &b) == kRecvOverlap)
      return fail(MPJX_ERR_ARG, "receive: %lld items of datatype %d (extent %lld) share a byte: they can be sent, not "
                  "received into", (long long)count, type, (long long)f.extent());
  }
  *out = q;
  return MPJX_SUCCESS;
}

// Posts q: a ready event unless the stream is idle, then the mailbox
int post(mpjx_comm* c, SmpTransport* t, hipStream_t s, const std::shared_ptr<P2PReq>& q) {
  if (q->peer != MPJX_PROC_NULL && q->bytes > 0 && hipStreamQuery(s) != hipSuccess) {
    (void)hipGetLastError();
    CHK(record_event(s, &q->ready));
  }
  (void)c;
  t->w->mail->post(q);
  return MPJX_SUCCESS;
}

mpjx_request* handle_of(mpjx_comm* c, SmpTransport* t, const std::shared_ptr<P2PReq>& q) {
  auto* h = new mpjx_request;
  h->q = q;
  h->c = c;
  h->w = t->w;
  h->alive = c->p2p_alive;
  return h;
}

int launch_error(hipError_t e) {
  if (e == hipErrorNoBinaryForGpu || e == hipErrorInvalidDeviceFunction)
    return fail(MPJX_ERR_NO_DEVICE, "no gfx950 kernel image for this device: %s", hipGetErrorString(e));
  if (e != hipSuccess) return fail(MPJX_ERR_HIP, "point-to-point launch: %s", hipGetErrorString(e));
  return MPJX_SUCCESS;
}

// True for a pair of two persistent requests: its segment is the same at every start
bool pooled_kind(const P2PPair& p) { return p.s->serial != 0 && p.r->serial != 0; }

// The batch through k_msgs_pool if every pair that moves bytes has its segment in c's pool: one launch per
// kPoolBatchMax pairs. *done = false (and nothing enqueued) otherwise.
int move_pooled(mpjx_comm* c, hipStream_t s, const std::vector<std::shared_ptr<P2PPair>>& batch, bool* done) {
  *done = false;
  if (!c->p2p_pool) return MPJX_SUCCESS;
  std::vector<const PoolMap::Entry*> hit;
  int64_t total = 0;
  for (const auto& p : batch) {
    if (p->wire != kPairPlain) return MPJX_SUCCESS;  // never pooled: the batch takes the table path
    if (p->s->bytes <= 0) continue;
    const PoolMap::Entry* e = pooled_kind(*p) ? c->p2p_pool_map.find(p->s->serial, p->r->serial) : nullptr;
    if (!e) return MPJX_SUCCESS;
    hit.push_back(e);
    total += e->bytes;
  }
  if (hit.empty()) return MPJX_SUCCESS;
  for (const auto& p : batch) {
    if (p->s->bytes <= 0) continue;
    for (const P2PReq* q : {p->s.get(), p->r.get()})
      if (q->rank != c->rank && q->ready) HIPCHK(hipStreamWaitEvent(s, event_of(q->ready), 0));
  }
  const bool nt = total >= kStridedStreamBytes;
  std::vector<PoolRef> refs;
  refs.reserve(hit.size());
  for (const PoolMap::Entry* e : hit) refs.push_back(PoolRef{e->slot, nt ? e->tiles_nt : e->tiles});
  int64_t launches = 0;
  CHK(launch_error(launch_msgs_pool(c->p2p_pool, refs, nt, s, &launches)));
  c->p2p_launches += launches;
  c->p2p_pool_launches += launches;
  c->p2p_pool_hits += (int64_t)hit.size();
  *done = true;
  return MPJX_SUCCESS;
}

// Stores the segments of the batch's newly met pairs of persistent requests into free slots of c's pool. The
// batch itself is enqueued already: a put that cannot be made (no memory for the pool, a failed launch) leaves
// its pairs unpooled, on the table path, and is no error of the exchange.
void pool_put(mpjx_comm* c, hipStream_t s, const std::vector<std::pair<const P2PPair*, MsgSeg>>& fresh) {
  std::vector<std::pair<MsgSeg, int>> puts;
  std::vector<const P2PPair*> put_pairs;
  for (const auto& f : fresh) {
    const P2PReq &a = *f.first->s, &b = *f.first->r;
    if (c->p2p_pool_map.find(a.serial, b.serial)) continue;
    if (!c->p2p_pool) {
      if (!PoolMap::poolable(f.second)) continue;
      if (hipMalloc((void**)&c->p2p_pool, sizeof(MsgSeg) * (size_t)kPoolSlots) != hipSuccess) {
        (void)hipGetLastError();
        c->p2p_pool = nullptr;
        return;
      }
    }
    const int slot = c->p2p_pool_map.put(a.serial, b.serial, f.second, a.freed, b.freed);
    if (slot < 0) continue;
    puts.emplace_back(f.second, slot);
    put_pairs.push_back(f.first);
  }
  if (puts.empty()) return;
  if (launch_msgs_pool_put(c->p2p_pool, puts, s) != hipSuccess) {
    (void)hipGetLastError();
    for (const P2PPair* p : put_pairs) c->p2p_pool_map.erase(p->s->serial, p->r->serial);  // never looked up unwritten
    return;
  }
  c->p2p_pool_puts += (int64_t)puts.size();
}

// The result slots of the unpack pairs: 8-byte cells of pinned host memory, 512 to a page, which the kernel
// stores with an ordinary store and the host reads without a copy. A slot lives as long as its pair, a page until
// its communicator and its last slot are gone; taken on the mover's thread, given back on whichever drops the pair.
struct WireSlotPage {
  std::mutex mu;
  uint64_t* cells = nullptr;
  std::vector<int> free_cells;
  static constexpr int kCells = 512;
  ~WireSlotPage() {
    if (cells) (void)hipHostFree(cells);
  }
};

int wire_slot(mpjx_comm* c, std::shared_ptr<void>* out) {
  std::shared_ptr<WireSlotPage> page;
  int cell = -1;
  for (const auto& v : c->p2p_wire_pages) {
    auto pg = std::static_pointer_cast<WireSlotPage>(v);
    std::lock_guard<std::mutex> g(pg->mu);
    if (!pg->free_cells.empty()) {
      cell = pg->free_cells.back();
      pg->free_cells.pop_back();
      page = pg;
      break;
    }
  }
  if (!page) {
    page = std::make_shared<WireSlotPage>();
    HIPCHK(hipHostMalloc((void**)&page->cells, sizeof(uint64_t) * WireSlotPage::kCells, hipHostMallocDefault));
    for (int i = WireSlotPage::kCells - 1; i >= 1; i--) page->free_cells.push_back(i);
    cell = 0;
    c->p2p_wire_pages.push_back(page);
  }
  uint64_t* at = page->cells + cell;
  *at = 0;
  *out = std::shared_ptr<void>(at, [page, cell](void*) {
    std::lock_guard<std::mutex> g(page->mu);
    page->free_cells.push_back(cell);
  });
  return MPJX_SUCCESS;
}

// The outcome of an unpack pair whose batch has completed on the host's view: the slot's {code, n} into the pair
void resolve_wire(Mailbox& mb, const std::shared_ptr<P2PPair>& p) {
  if (!p || p->wire != kPairUnpack || p->state != kPairLaunched || !p->slot) return;
  const volatile int32_t* v = static_cast<const volatile int32_t*>(p->slot.get());
  mb.resolve(*p, v[0], v[1]);
}

// The batch's segments onto `s`: the peers' ready events first
int move_batch(mpjx_comm* c, SmpTransport* t, hipStream_t s, const std::vector<std::shared_ptr<P2PPair>>& batch) {
  const bool pool_on = t->w->mail->batch && t->w->mail->seg_pool;
  if (pool_on) {
    bool done = false;
    CHK(move_pooled(c, s, batch, &done));
    if (done) return MPJX_SUCCESS;
  }
  std::vector<std::pair<const P2PPair*, MsgSeg>> fresh;
  std::vector<MsgSeg> segs;
  std::vector<TransposeSeg> tps;
  std::vector<std::pair<SideBytes, SideBytes>> plain;
  std::vector<WireSeg> wires;
  int64_t packs = 0, unpacks = 0;
  const bool batched = t->w->mail->batch;
  const bool tr_on = p2p_transpose_on();
  std::string err;
  for (const auto& p : batch) {
    if (p->wire != kPairPlain) {  // typed <-> PACKED: k_wire, under MPJX_P2P_BATCH=0 too (k_pack cannot take a short message)
      for (const P2PReq* q : {p->s.get(), p->r.get()})
        if (q->rank != c->rank && q->ready) HIPCHK(hipStreamWaitEvent(s, event_of(q->ready), 0));
      const bool un = p->wire == kPairUnpack;
      const P2PReq &typed = un ? *p->r : *p->s, &image = un ? *p->s : *p->r;
      const IdxEnt* tab = nullptr;
      if (typed.bytes > 0) CHK(p2p_idx_table(c, typed.lay, s, &tab));
      // a pack's section has at most 2^31 - 1 words; a receive layout may be longer than any section
      if (typed.bytes > 0 &&
          (typed.bytes >> strided_granule_log(typed.lay, mpjx::packed_side(image.lay.base + 8, typed.bytes))) > kStridedMaxGran)
        return fail(MPJX_ERR_UNSUPPORTED, "a layout of %lld bytes with MPI.PACKED on the other side exceeds 2^32 - 1 granules",
                    (long long)typed.bytes);
      WireSeg ws;
      if (un) {
        CHK(wire_slot(c, &p->slot));
        plan_wire_unpack(typed.lay, tab, image.lay.base, image.bytes, typed.base, typed.bsz,
                         (uint64_t)(uintptr_t)p->slot.get(), &ws);
        unpacks++;
      } else {
        plan_wire_pack(typed.lay, tab, image.lay.base, typed.base, typed.bsz, &ws);
        packs++;
      }
      wires.push_back(ws);
      continue;
    }
    if (p->s->bytes <= 0) continue;
    for (const P2PReq* q : {p->s.get(), p->r.get()})
      if (q->rank != c->rank && q->ready) HIPCHK(hipStreamWaitEvent(s, event_of(q->ready), 0));
    const SideBytes &a = p->s->lay, &b = p->r->lay;
    if (!batched) {
      plain.emplace_back(a, b);
      continue;
    }
    TransposeSeg ts;
    if (!(a.contiguous() && b.contiguous()) && a.regular() && b.regular() && a.total() == b.total() && tr_on &&
        plan_transpose_seg(a, b, &ts)) {
      tps.push_back(ts);
      continue;
    }
    const IdxEnt *stab, *dtab;
    CHK(p2p_idx_table(c, a, s, &stab));
    CHK(p2p_idx_table(c, b, s, &dtab));
    MsgSeg m{};
    const int rc = plan_msg_seg(a, stab, b, dtab, &m, &err);
    if (rc != kTypeOk) return fail(rc, "%s", err.c_str());
    segs.push_back(m);
    if (pool_on && pooled_kind(*p)) fresh.emplace_back(p.get(), m);
  }
  if (!wires.empty()) {
    int64_t n = 0;
    CHK(launch_error(launch_wire(wires, s, &n)));
    c->p2p_launches += n;
    c->p2p_wire_launches += n;
    c->p2p_wire_packed += packs;
    c->p2p_wire_unpacked += unpacks;
  }
  if (!batched) return p2p_launch_families(c, s, plain);
  hipError_t e = launch_msgs(segs, s, &c->p2p_launches);
  if (e == hipSuccess && !tps.empty()) {
    e = launch_transpose(tps, s);
    c->p2p_launches += ((int64_t)tps.size() + kTransposeMax - 1) / kTransposeMax;
  }
  CHK(launch_error(e));
  if (!fresh.empty()) pool_put(c, s, fresh);
  return MPJX_SUCCESS;
}

// Claims and moves every matched pair this rank is a party to
int progress(mpjx_comm* c, SmpTransport* t, hipStream_t s) {
  std::vector<std::shared_ptr<P2PPair>> batch;
  Mailbox& mb = *t->w->mail;
  mb.claim(c->rank, &batch);
  if (batch.empty()) return MPJX_SUCCESS;
  std::shared_ptr<void> done;
  int rc = move_batch(c, t, s, batch);
  if (rc == MPJX_SUCCESS) rc = record_event(s, &done);
  if (rc != MPJX_SUCCESS) {
    mb.launched(batch, nullptr, rc, mpjx_last_error());
    return rc;
  }
  c->p2p_moved += (int64_t)batch.size();
  mb.launched(batch, done);
  return MPJX_SUCCESS;
}

void fill(mpjx_status* out, const P2PStatus& st) {
  if (!out) return;
  out->source = st.source;
  out->tag = st.tag;
  out->error = st.error;
  out->elements = st.elements;
  out->bytes = st.bytes;
}

// The handle is done with: a plain request is deleted and *r is NULL; a persistent one stays, inactive (its
// activation is withdrawn if unmatched, its pair let go)
void drop(mpjx_request_t* r) {
  mpjx_request* h = *r;
  if (!h) return;
  if (h->pr) {
    h->pr->finish(h->w ? h->w->mail.get() : nullptr);
    return;
  }
  if (h->w && h->w->mail) {
    h->w->mail->withdraw(h->q);
    h->w->mail->release(h->q);
  }
  delete h;
  *r = nullptr;
}

// The posted request behind a handle: a plain handle's own, a persistent one's current activation (none while
// it is inactive). Persist::act is the only record of whether a persistent request is active.
const std::shared_ptr<P2PReq>& req_of(const mpjx_request* h) { return h->pr ? h->pr->act : h->q; }

// A NULL handle or an inactive persistent request: complete, with the empty status
bool idle(const mpjx_request* h) { return !h || !req_of(h); }

Mailbox::Clock::time_point deadline_of(mpjx_comm* c, SmpTransport* t) {
  const double sec = c->p2p_timeout_s > 0 ? c->p2p_timeout_s : t->w->mail->timeout_s;
  return Mailbox::Clock::now() + std::chrono::duration_cast<Mailbox::Clock::duration>(std::chrono::duration<double>(sec));
}

// Waits for n requests of one communicator (NULL handles and inactive persistent requests are skipped). On
// return every plain handle is NULL and every persistent one inactive.
int wait_many(int n, mpjx_request_t* reqs, mpjx_status* statuses) {
  mpjx_comm* c = nullptr;
  for (int i = 0; i < n; i++) {
    if (statuses) fill(&statuses[i], P2PStatus{});
    mpjx_request* h = reqs[i];
    if (idle(h)) continue;
    if (!h->alive->load()) {
      for (int j = 0; j < n; j++) drop(&reqs[j]);
      return fail(MPJX_ERR_INTERNAL, "the request's communicator was destroyed while it was pending");
    }
    if (c && h->c != c) return fail(MPJX_ERR_ARG, "the requests of one wait must belong to one communicator");
    c = h->c;
  }
  if (!c) return MPJX_SUCCESS;
  SmpTransport* t = nullptr;
  hipStream_t s = nullptr;
  int rc = p2p_world(c, &t);
  if (rc == MPJX_SUCCESS) rc = p2p_begin(c, &s);
  if (rc != MPJX_SUCCESS) {
    for (int j = 0; j < n; j++) drop(&reqs[j]);
    return rc;
  }
  Mailbox& mb = *t->w->mail;
  const auto deadline = deadline_of(c, t);
  for (int i = 0; i < n && rc == MPJX_SUCCESS; i++) {
    if (idle(reqs[i])) continue;
    const std::shared_ptr<P2PReq> q = req_of(reqs[i]);
    for (;;) {
      rc = progress(c, t, s);
      if (rc != MPJX_SUCCESS) break;
      const Mailbox::Wake w = mb.wait(q, deadline, &t->w->failed);
      if (w == Mailbox::kWakeMatched) continue;
      if (w == Mailbox::kWakeSettled) break;
      const std::string env = q->envelope();
      if (w == Mailbox::kWakeFailed)
        rc = fail(MPJX_ERR_INTERNAL, "multicore world: another rank failed while %s was pending", env.c_str());
      else
        rc = fail(MPJX_ERR_INTERNAL, "point-to-point wait timed out: %s was not %s within the limit", env.c_str(),
                  q->pair ? "moved by the rank that claimed it" : "matched");
      break;
    }
  }
  if (rc != MPJX_SUCCESS) {
    const std::string msg = mpjx_last_error();
    for (int j = 0; j < n; j++) drop(&reqs[j]);
    c->tr->call_failed();  // every peer's wait and later call errors out: no rank hangs
    mb.notify();
    return fail(rc, "%s", msg.c_str());
  }
  // every request is settled: order the stream after the batches other ranks moved, then drain it
  for (int i = 0; i < n; i++) {
    if (idle(reqs[i])) continue;
    const std::shared_ptr<P2PPair> p = req_of(reqs[i])->pair;
    if (p && p->state == kPairLaunched && p->mover != c->rank && p->done) {
      const hipError_t e = hipStreamWaitEvent(s, event_of(p->done), 0);
      if (e != hipSuccess && rc == MPJX_SUCCESS) rc = fail(MPJX_ERR_HIP, "hipStreamWaitEvent: %s", hipGetErrorString(e));
    }
  }
  if (rc == MPJX_SUCCESS) rc = c->tr->wait(s);
  c->last_stream = nullptr;  // complete on the host's view: whatever comes next is ordered after it
  c->last_recorded = false;
  std::string first;
  for (int i = 0; i < n; i++) {
    if (idle(reqs[i])) continue;
    const std::shared_ptr<P2PReq> q = req_of(reqs[i]);
    if (q->orphan && !q->pair && rc == MPJX_SUCCESS) {
      rc = MPJX_ERR_INTERNAL;
      first = "the request was withdrawn: " + q->envelope();
    }
    if (rc == MPJX_SUCCESS) resolve_wire(mb, q->pair);  // the batch's completion event has passed
    const P2PStatus st = p2p_status(*q);
    if (statuses) fill(&statuses[i], st);
    if (st.error != kP2POk && rc == MPJX_SUCCESS) {
      rc = st.error;
      first = q->pair->msg;
    }
    drop(&reqs[i]);
  }
  if (rc != MPJX_SUCCESS && !first.empty()) return fail(rc, "%s", first.c_str());
  return rc;
}

SideBytes packed_side(const char* p, int64_t bytes) {
  SideBytes x;
  x.base = (uint64_t)(uintptr_t)p;
  x.bb = x.sb = x.eb = bytes;
  x.nb = x.items = 1;
  return x;
}

// Packs q's layout to `at` on s and makes q a contiguous message from there
int pack_to(mpjx_comm* c, SmpTransport* t, hipStream_t s, const std::shared_ptr<P2PReq>& q, char* at) {
  auto tmp = std::make_shared<P2PPair>();
  tmp->s = q;
  tmp->r = std::make_shared<P2PReq>(*q);
  tmp->r->lay = packed_side(at, q->bytes);
  tmp->r->ready.reset();
  CHK(move_batch(c, t, s, {tmp}));
  q->lay = tmp->r->lay;
  return MPJX_SUCCESS;
}

// True once the eager message of q needs its chunk no longer (called under the mailbox lock)
bool chunk_done(const std::shared_ptr<P2PReq>& q) {
  bool done = q->consumed || q->orphan;
  if (!done && q->pair) {
    const P2PPair& p = *q->pair;
    done = p.state == kPairFailed || (p.state == kPairLaunched && (!p.done || hipEventQuery(event_of(p.done)) == hipSuccess));
    (void)hipGetLastError();
  }
  if (done) q->pair.reset();
  return done;
}

int isend_impl(mpjx_comm* c, const void* buf, int64_t count, int type, int dest, int tag, mpjx_request_t* request,
               bool eager_ok, bool* went_eager) {
  SmpTransport* t = nullptr;
  CHK(p2p_world(c, &t));
  std::shared_ptr<P2PReq> q;
  CHK(plan_req(c, true, buf, count, type, dest, tag, &q));
  hipStream_t s = nullptr;
  CHK(p2p_begin(c, &s));
  Mailbox& mb = *t->w->mail;
  if (went_eager) *went_eager = false;
  if (eager_ok && dest != MPJX_PROC_NULL && q->bytes <= mb.eager_bytes) {
    int64_t off = 0;
    if (q->bytes > 0) {
      if (!c->p2p_slab) {
        HIPCHK(hipMalloc((void**)&c->p2p_slab, (size_t)mb.pool_bytes));
        c->p2p_chunks = EagerSlab(mb.pool_bytes);
      }
      std::lock_guard<std::mutex> g(mb.mutex());
      off = c->p2p_chunks.alloc(q->bytes, q, chunk_done);
    }
    if (off >= 0) {
      q->eager = true;
      if (q->bytes > 0) CHK(pack_to(c, t, s, q, c->p2p_slab + off));
      CHK(post(c, t, s, q));
      c->p2p_eager++;
      if (went_eager) *went_eager = true;
      return MPJX_SUCCESS;
    }
  }
  CHK(post(c, t, s, q));
  *request = handle_of(c, t, q);
  return MPJX_SUCCESS;
}

int irecv_impl(mpjx_comm* c, void* buf, int64_t count, int type, int source, int tag, mpjx_request_t* request) {
  SmpTransport* t = nullptr;
  CHK(p2p_world(c, &t));
  std::shared_ptr<P2PReq> q;
  CHK(plan_req(c, false, buf, count, type, source, tag, &q));
  hipStream_t s = nullptr;
  CHK(p2p_begin(c, &s));
  CHK(post(c, t, s, q));
  *request = handle_of(c, t, q);
  return MPJX_SUCCESS;
}

}  // namespace

namespace mpjx {

std::shared_ptr<Mailbox> p2p_make_mailbox(int P) {
  auto mb = std::make_shared<Mailbox>(P);
  mb->timeout_s = env_double("MPJX_P2P_TIMEOUT_S", 300);
  mb->eager_bytes = (int64_t)(env_double("MPJX_P2P_EAGER_KIB", 128) * 1024);
  mb->pool_bytes = (int64_t)env_double("MPJX_P2P_EAGER_POOL_MIB", 8) << 20;
  const char* e = getenv("MPJX_P2P_BATCH");
  mb->batch = !(e && e[0] == '0' && e[1] == 0);
  e = getenv("MPJX_P2P_POOL");
  mb->seg_pool = !(e && e[0] == '0' && e[1] == 0);
  return mb;
}

void p2p_comm_destroy(mpjx_comm* c) {
  c->p2p_alive->store(false);
  auto* t = dynamic_cast<SmpTransport*>(c->tr.get());
  if (t && t->w->mail) {
    t->w->mail->retire_rank(c->rank);
    std::lock_guard<std::mutex> g(t->w->mail->mutex());
    c->p2p_chunks.clear([](const std::shared_ptr<P2PReq>& q) { q->pair.reset(); });
  }
  if (c->p2p_slab) (void)hipFree(c->p2p_slab);
  c->p2p_slab = nullptr;
  if (c->p2p_pool) (void)hipFree(c->p2p_pool);
  c->p2p_pool = nullptr;
}

}  // namespace mpjx

extern "C" int mpjx_isend(mpjx_comm_t c, const void* buf, int64_t count, int type, int dest, int tag,
                          mpjx_request_t* request) {
  COMM_ARG(c);
  if (!request) return fail(MPJX_ERR_ARG, "request is NULL");
  *request = nullptr;
  return isend_impl(c, buf, count, type, dest, tag, request, false, nullptr);
}

extern "C" int mpjx_irecv(mpjx_comm_t c, void* buf, int64_t count, int type, int source, int tag,
                          mpjx_request_t* request) {
  COMM_ARG(c);
  if (!request) return fail(MPJX_ERR_ARG, "request is NULL");
  *request = nullptr;
  return irecv_impl(c, buf, count, type, source, tag, request);
}

extern "C" int mpjx_send(mpjx_comm_t c, const void* buf, int64_t count, int type, int dest, int tag) {
  COMM_ARG(c);
  mpjx_request_t r = nullptr;
  bool eager = false;
  CHK(isend_impl(c, buf, count, type, dest, tag, &r, true, &eager));
  return eager ? MPJX_SUCCESS : wait_many(1, &r, nullptr);
}

extern "C" int mpjx_recv(mpjx_comm_t c, void* buf, int64_t count, int type, int source, int tag, mpjx_status* status) {
  COMM_ARG(c);
  mpjx_request_t r = nullptr;
  CHK(irecv_impl(c, buf, count, type, source, tag, &r));
  return wait_many(1, &r, status);
}

extern "C" int mpjx_sendrecv(mpjx_comm_t c, const void* sendbuf, int64_t sendcount, int sendtype, int dest, int sendtag,
                             void* recvbuf, int64_t recvcount, int recvtype, int source, int recvtag,
                             mpjx_status* status) {
  COMM_ARG(c);
  // Comm.java:2334-2343: Irecv, Isend, wait for both. Both are checked before either is posted.
  SmpTransport* t = nullptr;
  CHK(p2p_world(c, &t));
  std::shared_ptr<P2PReq> probe;
  CHK(plan_req(c, true, sendbuf, sendcount, sendtype, dest, sendtag, &probe));
  mpjx_request_t r[2] = {nullptr, nullptr};
  CHK(irecv_impl(c, recvbuf, recvcount, recvtype, source, recvtag, &r[0]));
  const int rc = isend_impl(c, sendbuf, sendcount, sendtype, dest, sendtag, &r[1], false, nullptr);
  if (rc != MPJX_SUCCESS) {
    drop(&r[0]);
    return rc;
  }
  mpjx_status st[2];
  const int wrc = wait_many(2, r, st);
  if (status) *status = st[0];
  return wrc;
}

extern "C" int mpjx_sendrecv_replace(mpjx_comm_t c, void* buf, int64_t count, int type, int dest, int sendtag,
                                     int source, int recvtag, mpjx_status* status) {
  COMM_ARG(c);
  SmpTransport* t = nullptr;
  CHK(p2p_world(c, &t));
  std::shared_ptr<P2PReq> sq, rq;
  CHK(plan_req(c, true, buf, count, type, dest, sendtag, &sq));
  CHK(plan_req(c, false, buf, count, type, source, recvtag, &rq));
  hipStream_t s = nullptr;
  CHK(p2p_begin(c, &s));
  // the outgoing message leaves from the communicator's staging, so the incoming one may land in buf
  if (sq->bytes > 0 && dest != MPJX_PROC_NULL) {
    CHK(grow_device(c, &c->dtstage, &c->dtstage_bytes, (size_t)sq->bytes, s));
    CHK(pack_to(c, t, s, sq, c->dtstage));
  }
  CHK(post(c, t, s, rq));
  mpjx_request_t r[2] = {handle_of(c, t, rq), nullptr};
  const int rc = post(c, t, s, sq);
  if (rc != MPJX_SUCCESS) {
    drop(&r[0]);
    return rc;
  }
  r[1] = handle_of(c, t, sq);
  mpjx_status st[2];
  const int wrc = wait_many(2, r, st);
  if (status) *status = st[0];
  return wrc;
}

extern "C" int mpjx_wait(mpjx_request_t* request, mpjx_status* status) {
  if (!request) return fail(MPJX_ERR_ARG, "request is NULL");
  return wait_many(1, request, status);
}

extern "C" int mpjx_waitall(int n, mpjx_request_t* requests, mpjx_status* statuses) {
  if (n < 0 || (n > 0 && !requests)) return fail(MPJX_ERR_ARG, "bad request list (n = %d)", n);
  return wait_many(n, requests, statuses);
}

extern "C" int mpjx_test(mpjx_request_t* request, int* flag, mpjx_status* status) {
  if (!request || !flag) return fail(MPJX_ERR_ARG, "NULL argument");
  *flag = 0;
  fill(status, P2PStatus{});
  mpjx_request* h = *request;
  if (idle(h)) {
    *flag = 1;
    return MPJX_SUCCESS;
  }
  if (!h->alive->load()) {
    drop(request);
    return fail(MPJX_ERR_INTERNAL, "the request's communicator was destroyed while it was pending");
  }
  mpjx_comm* c = h->c;
  SmpTransport* t = nullptr;
  hipStream_t s = nullptr;
  CHK(p2p_world(c, &t));
  CHK(p2p_begin(c, &s));
  CHK(progress(c, t, s));
  const std::shared_ptr<P2PReq> q = req_of(h);
  if (!t->w->mail->settled(q)) return MPJX_SUCCESS;
  const std::shared_ptr<P2PPair> p = q->pair;
  if (p && p->state == kPairLaunched && p->done) {
    const hipError_t e = hipEventQuery(event_of(p->done));
    if (e == hipErrorNotReady) {
      (void)hipGetLastError();
      return MPJX_SUCCESS;
    }
    if (e != hipSuccess) return fail(MPJX_ERR_HIP, "hipEventQuery: %s", hipGetErrorString(e));
  }
  resolve_wire(*t->w->mail, p);
  const P2PStatus st = p2p_status(*q);
  const std::string msg = p ? p->msg : std::string();
  fill(status, st);
  *flag = 1;
  drop(request);
  return st.error == kP2POk ? MPJX_SUCCESS : fail(st.error, "%s", msg.c_str());
}

extern "C" int mpjx_request_free(mpjx_request_t* request) {
  if (!request) return fail(MPJX_ERR_ARG, "request is NULL");
  if (*request && (*request)->pr) {  // Prequest.Free: a pending activation is withdrawn or orphaned, then the plan goes
    mpjx_request* h = *request;
    drop(request);
    delete h;
    *request = nullptr;
    return MPJX_SUCCESS;
  }
  drop(request);
  return MPJX_SUCCESS;
}

// ---- persistent requests (src/mpi/Prequest.java; Comm.java Send_init / Recv_init) ---------------------------------

namespace {

// Send_init / Recv_init. What can be judged from the arguments alone is judged first (as mpjx_pack does), so a
// NULL request, a negative count and a negative tag are MPJX_ERR_ARG whatever the communicator is, NULL included.
int init_impl(mpjx_comm* c, bool send, const void* buf, int64_t count, int type, int peer, int tag,
              mpjx_request_t* request) {
  const char* who = send ? "mpjx_send_init" : "mpjx_recv_init";
  if (!request) return fail(MPJX_ERR_ARG, "%s: request is NULL", who);
  *request = nullptr;
  if (count < 0) return fail(MPJX_ERR_ARG, "%s: negative count %lld", who, (long long)count);
  if (tag < 0 && !(!send && tag == MPJX_ANY_TAG)) return fail(MPJX_ERR_ARG, "%s: tag %d is negative", who, tag);
  COMM_ARG(c);
  SmpTransport* t = nullptr;
  CHK(p2p_world(c, &t));
  std::shared_ptr<P2PReq> q;
  CHK(plan_req(c, send, buf, count, type, peer, tag, &q));
  mpjx_request* h = handle_of(c, t, nullptr);
  h->pr = std::make_shared<Persist>(*q);
  *request = h;
  return MPJX_SUCCESS;
}

// The checks of Start on one handle; `what` names the call
int startable(const mpjx_request* h, const char* what) {
  if (!h) return fail(MPJX_ERR_ARG, "%s: the request is NULL", what);
  if (!h->pr) return fail(MPJX_ERR_ARG, "%s: not a persistent request (it was made by Isend or Irecv)", what);
  if (h->pr->act)
    return fail(MPJX_ERR_ARG, "%s: the request is active: %s has not completed", what, h->pr->act->envelope().c_str());
  if (!h->alive->load()) return fail(MPJX_ERR_INTERNAL, "%s: the request's communicator was destroyed", what);
  return MPJX_SUCCESS;
}

// Activates the n checked handles of communicator c (NULL entries skipped): one p2p_begin, one stream query, at
// most one ready event shared by all, one acquisition of the mailbox lock, array order
int start_many(mpjx_comm* c, int n, mpjx_request_t* reqs) {
  SmpTransport* t = nullptr;
  hipStream_t s = nullptr;
  CHK(p2p_world(c, &t));
  CHK(p2p_begin(c, &s));
  bool moves = false;
  for (int i = 0; i < n && !moves; i++)
    moves = reqs[i] && reqs[i]->pr->plan.peer != MPJX_PROC_NULL && reqs[i]->pr->plan.bytes > 0;
  std::shared_ptr<void> ready;
  if (moves && hipStreamQuery(s) != hipSuccess) {
    (void)hipGetLastError();
    CHK(record_event(s, &ready));
  }
  std::vector<std::shared_ptr<P2PReq>> acts;
  acts.reserve((size_t)n);
  for (int i = 0; i < n; i++) {
    if (!reqs[i]) continue;
    std::shared_ptr<P2PReq> q = reqs[i]->pr->start();
    if (!q) {  // active after all (startable() rules it out): post what was started, so that no handle is left half done
      t->w->mail->post_all(acts);
      return fail(MPJX_ERR_INTERNAL, "mpjx_start: request %d became active while the list was being started", i);
    }
    if (q->peer != MPJX_PROC_NULL && q->bytes > 0) q->ready = ready;
    acts.push_back(std::move(q));
  }
  t->w->mail->post_all(acts);
  return MPJX_SUCCESS;
}

}  // namespace

extern "C" int mpjx_send_init(mpjx_comm_t c, const void* buf, int64_t count, int type, int dest, int tag,
                              mpjx_request_t* request) {
  return init_impl(c, true, buf, count, type, dest, tag, request);
}

extern "C" int mpjx_recv_init(mpjx_comm_t c, void* buf, int64_t count, int type, int source, int tag,
                              mpjx_request_t* request) {
  return init_impl(c, false, buf, count, type, source, tag, request);
}

extern "C" int mpjx_start(mpjx_request_t* request) {
  if (!request) return fail(MPJX_ERR_ARG, "mpjx_start: request is NULL");
  CHK(startable(*request, "mpjx_start"));
  return start_many((*request)->c, 1, request);
}

extern "C" int mpjx_startall(int n, mpjx_request_t* requests) {
  if (n < 0 || (n > 0 && !requests)) return fail(MPJX_ERR_ARG, "bad request list (n = %d)", n);
  mpjx_comm* c = nullptr;
  for (int i = 0; i < n; i++) {
    if (!requests[i]) continue;
    CHK(startable(requests[i], "mpjx_startall"));
    if (c && requests[i]->c != c) return fail(MPJX_ERR_ARG, "the requests of one mpjx_startall must belong to one communicator");
    c = requests[i]->c;
    for (int j = 0; j < i; j++)
      if (requests[j] == requests[i]) return fail(MPJX_ERR_ARG, "mpjx_startall: request %d appears twice in the list", i);
  }
  return c ? start_many(c, n, requests) : MPJX_SUCCESS;
}

extern "C" int mpjx_request_is_persistent(mpjx_request_t request, int* persistent, int* active) {
  if (persistent) *persistent = request && request->pr ? 1 : 0;
  if (active) *active = request && request->pr && request->pr->act ? 1 : 0;
  return MPJX_SUCCESS;
}

extern "C" int mpjx_comm_p2p_pool_stats(mpjx_comm_t c, int64_t* pool_launches, int64_t* puts, int64_t* hits,
                                        int64_t* slots_in_use, int* batch_max) {
  SmpTransport* t = nullptr;
  CHK(p2p_world(c, &t, false));
  if (pool_launches) *pool_launches = c->p2p_pool_launches;
  if (puts) *puts = c->p2p_pool_puts;
  if (hits) *hits = c->p2p_pool_hits;
  if (slots_in_use) *slots_in_use = c->p2p_pool_map.in_use();
  if (batch_max) *batch_max = kPoolBatchMax;
  return MPJX_SUCCESS;
}

extern "C" int mpjx_get_count(const mpjx_status* status, int type, int64_t* count, int64_t* elements) {
  if (!status) return fail(MPJX_ERR_ARG, "status is NULL");
  TypeForm f;
  // MPI.PACKED counts bytes: a type of size 1
  if (!(type == MPJX_PACKED ? basic_form(MPJX_BYTE, &f) : type_form(type, &f)))
    return fail(MPJX_ERR_ARG, "mpjx_get_count: unknown or freed datatype code %d", type);
  int64_t cn = 0, el = 0;
  p2p_get_count(status->elements, f.size(), &cn, &el);
  if (count) *count = cn;
  if (elements) *elements = el;
  return MPJX_SUCCESS;
}

extern "C" int mpjx_comm_set_p2p_timeout(mpjx_comm_t c, double seconds) {
  SmpTransport* t = nullptr;
  CHK(p2p_world(c, &t, false));
  if (!(seconds > 0)) return fail(MPJX_ERR_ARG, "the timeout must be positive (%g)", seconds);
  c->p2p_timeout_s = seconds;
  return MPJX_SUCCESS;
}

extern "C" int mpjx_comm_p2p_stats(mpjx_comm_t c, int64_t* launches, int64_t* moved, int64_t* eager, int* table_max) {
  SmpTransport* t = nullptr;
  CHK(p2p_world(c, &t, false));
  if (launches) *launches = c->p2p_launches;
  if (moved) *moved = c->p2p_moved;
  if (eager) *eager = c->p2p_eager;
  if (table_max) *table_max = kMsgsMax;
  return MPJX_SUCCESS;
}

extern "C" int mpjx_comm_p2p_wire_stats(mpjx_comm_t c, int64_t* launches, int64_t* packed, int64_t* unpacked,
                                        int* table_max) {
  SmpTransport* t = nullptr;
  CHK(p2p_world(c, &t, false));
  if (launches) *launches = c->p2p_wire_launches;
  if (packed) *packed = c->p2p_wire_packed;
  if (unpacked) *unpacked = c->p2p_wire_unpacked;
  if (table_max) *table_max = kWireMax;
  return MPJX_SUCCESS;
}

// ---- Probe, Iprobe (src/mpi/Comm.java:1761, :1811) -----------------------------------------------------------------

namespace {

// Iprobe (block = false) and Probe. What can be judged from the arguments alone is judged first.
int probe_impl(mpjx_comm* c, int source, int tag, int* flag, mpjx_status* status, bool block) {
  const char* who = block ? "mpjx_probe" : "mpjx_iprobe";
  if (!block && !flag) return fail(MPJX_ERR_ARG, "%s: flag is NULL", who);
  if (flag) *flag = 0;
  fill(status, P2PStatus{});
  if (tag < 0 && tag != MPJX_ANY_TAG) return fail(MPJX_ERR_ARG, "%s: tag %d is negative", who, tag);
  COMM_ARG(c);
  SmpTransport* t = nullptr;
  CHK(p2p_world(c, &t));
  if (!(source >= 0 && source < c->size) && source != MPJX_PROC_NULL && source != MPJX_ANY_SOURCE)
    return fail(MPJX_ERR_ARG, "%s: rank %d out of range (the communicator has %d)", who, source, c->size);
  if (source == MPJX_PROC_NULL) {  // returns at once with the empty status
    if (flag) *flag = 1;
    return MPJX_SUCCESS;
  }
  Mailbox& mb = *t->w->mail;
  P2PStatus st;
  if (!block) {
    if (mb.peek(c->rank, source, tag, &st)) {
      *flag = 1;
      fill(status, st);
    }
    return MPJX_SUCCESS;
  }
  // a host wait: nothing is enqueued on the GPU
  const Mailbox::Wake w = mb.probe(c->rank, source, tag, deadline_of(c, t), &t->w->failed, &st);
  if (w == Mailbox::kWakeMatched) {
    fill(status, st);
    return MPJX_SUCCESS;
  }
  if (w == Mailbox::kWakeFailed)
    return fail(MPJX_ERR_INTERNAL, "multicore world: another rank failed while rank %d was probing", c->rank);
  const std::string what = "rank " + std::to_string(c->rank) + " <- " +
                           (source == MPJX_ANY_SOURCE ? std::string("ANY_SOURCE") : std::to_string(source)) + ", tag " +
                           (tag == MPJX_ANY_TAG ? std::string("ANY_TAG") : std::to_string(tag));
  c->tr->call_failed();  // every peer's wait and later call errors out: no rank hangs
  mb.notify();
  return fail(MPJX_ERR_INTERNAL, "point-to-point probe timed out: no message for (%s) within the limit", what.c_str());
}

}  // namespace

extern "C" int mpjx_iprobe(mpjx_comm_t c, int source, int tag, int* flag, mpjx_status* status) {
  return probe_impl(c, source, tag, flag, status, false);
}

extern "C" int mpjx_probe(mpjx_comm_t c, int source, int tag, mpjx_status* status) {
  return probe_impl(c, source, tag, nullptr, status, true);
}

extern "C" int mpjx_wire_bytes(const mpjx_status* status, int64_t* bytes) {
  if (!status || !bytes) return fail(MPJX_ERR_ARG, "mpjx_wire_bytes: NULL argument");
  if (status->bytes < 0) return fail(MPJX_ERR_ARG, "mpjx_wire_bytes: negative bytes %lld", (long long)status->bytes);
  // a typed message needs its section header; a PACKED one (elements unknown to the host) is an image already
  *bytes = status->elements == MPJX_UNDEFINED ? status->bytes : 8 + status->bytes;
  return MPJX_SUCCESS;
}
