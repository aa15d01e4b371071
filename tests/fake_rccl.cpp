// fake_rccl.cpp -- a test-only, in-process stand-in for the nine RCCL entry points librc2dgi resolves
// (rc2dgi_group.cpp: rccl()), so that the ranks of a row-strip frame can run as threads of one process on one
// device (tests/test_gpu_rccl_ranks.py).  Loaded through RC2DGI_RCCL_LIB; never linked against RCCL, no kernels,
// HIP runtime API only.  The signatures come from the installed <rccl/rccl.h>, so one that drifts fails to compile.
//
// Calling rules restated from the public NCCL / RCCL documentation:
//  - ncclGetUniqueId / ncclCommInitRank ("Creating a Communicator", api/comms): one id, every rank joins with the
//    same nranks and a distinct rank.  (The real call blocks until all ranks joined; this one does not, so one
//    thread may connect the ranks in turn.  Every operation waits for its peers instead.)
//  - ncclGroupStart / ncclGroupEnd ("Group Calls", usage/groups): nest per thread; the operations between them are
//    issued together at the outermost ncclGroupEnd; an operation outside a group is a group of one.
//  - ncclSend / ncclRecv ("Point-to-point communication", usage/p2p): a send matches the receive the peer posts
//    for it, in the order posted between that ordered pair of ranks, with the same count and type.
//  - ncclBroadcast ("Collective Operations", usage/collectives): every rank calls the collectives of a communicator
//    in the same order with the same root and count; only the root's sendbuff is read; sendbuff == recvbuff on the
//    root is the in-place form.
//  - Stream semantics ("CUDA Stream Semantics", usage/streams): an operation is enqueued on the caller's stream: it
//    starts after the work enqueued before it there and the stream's later work starts after it.
// Stricter than RCCL where RCCL leaves the result undefined: within one group of one rank a receive destination
// that overlaps another receive destination, a send source or a broadcast buffer of that group is an error.
// Every host-side wait has a limit (fake_rccl_set_wait_limit_ms, default 30 s); there is no device-side wait.
#pragma GCC visibility push(default)
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>
#pragma GCC visibility pop

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

struct ncclComm {  // (rccl.h leaves the type incomplete) one rank's handle on its in-process communicator
  struct World *w;
  int rank;
  bool alive;
};

namespace {

struct P2P {  // the nth transfer of an ordered pair (source, destination)
  bool has_send = false, has_recv = false, dead = false, done = false;
  const void *src = nullptr;
  size_t sbytes = 0, rbytes = 0;
  hipEvent_t ready = nullptr, fin = nullptr;  // source data ready on the sender's stream / copy done on the receiver's
};
struct Pair {
  long ns = 0, nr = 0;
  std::map<long, P2P> slot;
};
struct Coll {  // the nth collective of a communicator
  int posted = 0;
  bool dead = false;
  std::vector<char> has;
  std::vector<int> root;
  std::vector<size_t> bytes;
  const void *src = nullptr;
  hipEvent_t ready = nullptr;
  std::vector<hipEvent_t> fin;  // one per non-root rank whose copy is enqueued
};
struct LogEntry {
  const char *kind;
  int peer;
  size_t bytes;
  long group;
};

}  // namespace

struct World {
  int nranks = 0, live = 0;
  bool broken = false;  // a group failed on some rank: no wait on this communicator outlasts that
  std::vector<char> joined;
  std::map<std::pair<int, int>, Pair> pair;
  std::map<long, Coll> coll;
  std::vector<long> ncoll, groups;
  std::vector<std::vector<LogEntry>> log;
  std::vector<hipEvent_t> events;  // every event of this communicator; destroyed when its last rank leaves
};

namespace {

const char kMagic[8] = {'F', 'A', 'K', 'E', 'R', 'C', 'C', 'L'};
std::mutex g_mu;
std::condition_variable g_cv;
std::map<uint64_t, World> g_worlds;  // by token; kept (with their logs) for the life of the process
uint64_t g_next_token = 1;
std::atomic<long> g_limit_ms{30000};

struct Op {
  char kind;  // 's'end, 'r'ecv, 'b'roadcast
  ncclComm *c;
  const void *src;
  void *dst;
  size_t bytes;
  int peer;  // the peer, or the root
  hipStream_t st;
  P2P *p = nullptr;
  Coll *k = nullptr;
};
thread_local int t_depth = 0;
thread_local std::vector<Op> t_ops;
thread_local std::string t_detail, t_msg;

ncclResult_t err(ncclResult_t e, const std::string &detail) {
  t_detail = detail;
  return e;
}

std::string describe(const Op &o) {
  const char *kind = o.kind == 's' ? "send" : o.kind == 'r' ? "recv" : "broadcast";
  return std::string(kind) + " on rank " + std::to_string(o.c->rank) + (o.kind == 'b' ? ", root " : ", peer ") +
         std::to_string(o.peer) + ", " + std::to_string(o.bytes) + " bytes";
}

size_t type_size(ncclDataType_t t) {
  switch (t) {
    case ncclInt8: case ncclUint8: case ncclFloat8e4m3: case ncclFloat8e5m2: return 1;
    case ncclFloat16: case ncclBfloat16: return 2;
    case ncclInt32: case ncclUint32: case ncclFloat32: return 4;
    case ncclInt64: case ncclUint64: case ncclFloat64: return 8;
    default: return 0;
  }
}

bool overlap(const void *a, size_t na, const void *b, size_t nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return na && nb && x < y + nb && y < x + na;
}

// waits (g_mu held through lk) until pred() or the limit; false on expiry
template <class Pred>
bool wait_for(std::unique_lock<std::mutex> &lk, Pred pred) {
  return g_cv.wait_until(lk, std::chrono::steady_clock::now() + std::chrono::milliseconds(g_limit_ms.load()), pred);
}

hipEvent_t new_event(World *w, hipStream_t st, hipError_t &he) {  // g_mu held
  hipEvent_t ev = nullptr;
  he = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  if (he != hipSuccess) return nullptr;
  w->events.push_back(ev);
  he = hipEventRecord(ev, st);
  return ev;
}

// a group that failed leaves none of its operations for a peer to wait on
void abandon(std::vector<Op> &ops) {
  for (Op &o : ops) {
    if (o.p) o.p->dead = true;
    if (o.k) o.k->dead = true;
    o.c->w->broken = true;
  }
  g_cv.notify_all();
}

ncclResult_t check_overlaps(const std::vector<Op> &ops) {
  struct Range {
    const void *p;
    size_t n;
    bool written;
    const Op *o;
  };
  std::vector<Range> r;
  for (const Op &o : ops) {
    if (o.kind == 's') r.push_back({o.src, o.bytes, false, &o});
    if (o.kind == 'r') r.push_back({o.dst, o.bytes, true, &o});
    if (o.kind == 'b' && o.peer == o.c->rank) {
      r.push_back({o.src, o.bytes, false, &o});
      if (o.dst != o.src) r.push_back({o.dst, o.bytes, true, &o});
    } else if (o.kind == 'b') {
      r.push_back({o.dst, o.bytes, true, &o});
    }
  }
  for (size_t i = 0; i < r.size(); ++i)
    for (size_t j = i + 1; j < r.size(); ++j)
      if ((r[i].written || r[j].written) && r[i].o != r[j].o && overlap(r[i].p, r[i].n, r[j].p, r[j].n))
        return err(ncclInvalidUsage, "overlapping buffers in one group: " + describe(*r[i].o) + " and " + describe(*r[j].o));
  return ncclSuccess;
}

#define FAKE_HIP(expr)                                                                                      \
  do {                                                                                                      \
    const hipError_t he_ = (expr);                                                                          \
    if (he_ != hipSuccess) return err(ncclUnhandledCudaError, std::string(#expr ": ") + hipGetErrorString(he_)); \
  } while (0)

// the operations of one outermost group, g_mu held: publish everything, then the copies this rank receives, then
// the waits for the readers of what it sends
ncclResult_t run_locked(std::vector<Op> &ops, std::unique_lock<std::mutex> &lk) {
  // 1. one data-ready event per stream, then every operation posted before anything waits
  std::map<hipStream_t, hipEvent_t> ready;
  for (Op &o : ops) {
    if (ready.count(o.st)) continue;
    hipError_t he;
    ready[o.st] = new_event(o.c->w, o.st, he);
    FAKE_HIP(he);
  }
  for (Op &o : ops) {
    World *w = o.c->w;
    const int me = o.c->rank;
    if (o.kind == 's') {
      Pair &pr = w->pair[{me, o.peer}];
      o.p = &pr.slot[pr.ns++];
      o.p->has_send = true;
      o.p->src = o.src;
      o.p->sbytes = o.bytes;
      o.p->ready = ready[o.st];
    } else if (o.kind == 'r') {
      Pair &pr = w->pair[{o.peer, me}];
      o.p = &pr.slot[pr.nr++];
      o.p->has_recv = true;
      o.p->rbytes = o.bytes;
    } else {
      o.k = &w->coll[w->ncoll[me]++];
      if (o.k->has.empty()) {
        o.k->has.assign(w->nranks, 0);
        o.k->root.assign(w->nranks, -1);
        o.k->bytes.assign(w->nranks, 0);
      }
      o.k->has[me] = 1;
      o.k->root[me] = o.peer;
      o.k->bytes[me] = o.bytes;
      ++o.k->posted;
      if (o.peer == me) {
        o.k->src = o.src;
        o.k->ready = ready[o.st];
      }
    }
  }
  g_cv.notify_all();
  // 2. receives and broadcasts: wait for the peers' publication, then the copy on the own stream
  for (Op &o : ops) {
    World *w = o.c->w;
    const int me = o.c->rank;
    if (o.kind == 'r') {
      P2P *p = o.p;
      if (!wait_for(lk, [&] { return p->has_send || p->dead || w->broken; }))
        return err(ncclInternalError, "no matching send after the wait limit: " + describe(o));
      if (p->has_send && p->sbytes != p->rbytes)  // (both sides report it, whichever looks first)
        return err(ncclInvalidArgument, describe(o) + " matches a send of " + std::to_string(p->sbytes) + " bytes");
      if (!p->has_send || p->dead) return err(ncclInternalError, "the peer's group failed: " + describe(o));
      if (o.bytes) {
        FAKE_HIP(hipStreamWaitEvent(o.st, p->ready, 0));
        FAKE_HIP(hipMemcpyAsync(o.dst, p->src, o.bytes, hipMemcpyDeviceToDevice, o.st));
      }
      hipError_t he;
      p->fin = new_event(w, o.st, he);
      FAKE_HIP(he);
      p->done = true;
      g_cv.notify_all();
    } else if (o.kind == 'b') {
      Coll *k = o.k;
      if (!wait_for(lk, [&] { return k->posted == w->nranks || k->dead || w->broken; })) {
        std::string missing;
        for (int q = 0; q < w->nranks; ++q)
          if (!k->has[q]) missing += " " + std::to_string(q);
        return err(ncclInternalError, "ranks" + missing + " posted no matching collective after the wait limit: " + describe(o));
      }
      for (int q = 0; q < w->nranks; ++q)  // (every rank reports a disagreement, whichever looks first)
        if (k->has[q] && (k->root[q] != o.peer || k->bytes[q] != o.bytes))
          return err(ncclInvalidArgument, describe(o) + " matches rank " + std::to_string(q) + "'s with root " +
                                              std::to_string(k->root[q]) + ", " + std::to_string(k->bytes[q]) + " bytes");
      if (k->posted != w->nranks || k->dead) return err(ncclInternalError, "a peer's group failed: " + describe(o));
      if (o.peer == me) {
        if (o.dst != o.src && o.bytes) FAKE_HIP(hipMemcpyAsync(o.dst, o.src, o.bytes, hipMemcpyDeviceToDevice, o.st));
      } else {
        if (o.bytes) {
          FAKE_HIP(hipStreamWaitEvent(o.st, k->ready, 0));
          FAKE_HIP(hipMemcpyAsync(o.dst, k->src, o.bytes, hipMemcpyDeviceToDevice, o.st));
        }
        hipError_t he;
        hipEvent_t ev = new_event(w, o.st, he);
        FAKE_HIP(he);
        k->fin.push_back(ev);
        g_cv.notify_all();
      }
    }
  }
  // 3. sends and rooted broadcasts: later work on this stream starts after the readers' copies
  for (Op &o : ops) {
    World *w = o.c->w;
    if (o.kind == 's') {
      P2P *p = o.p;
      if (!wait_for(lk, [&] { return p->has_recv || p->dead || w->broken; }))
        return err(ncclInternalError, "no matching receive after the wait limit: " + describe(o));
      if (p->has_recv && p->sbytes != p->rbytes)
        return err(ncclInvalidArgument, describe(o) + " matches a receive of " + std::to_string(p->rbytes) + " bytes");
      if (!wait_for(lk, [&] { return p->done || p->dead || w->broken; }))
        return err(ncclInternalError, "the receiver did not finish after the wait limit: " + describe(o));
      if (!p->done) return err(ncclInternalError, "the peer's group failed: " + describe(o));
      FAKE_HIP(hipStreamWaitEvent(o.st, p->fin, 0));
    } else if (o.kind == 'b' && o.peer == o.c->rank) {
      Coll *k = o.k;
      if (!wait_for(lk, [&] { return (int)k->fin.size() == w->nranks - 1 || k->dead || w->broken; }))
        return err(ncclInternalError, "the readers did not finish after the wait limit: " + describe(o));
      if ((int)k->fin.size() != w->nranks - 1) return err(ncclInternalError, "a peer's group failed: " + describe(o));
      for (hipEvent_t ev : k->fin) FAKE_HIP(hipStreamWaitEvent(o.st, ev, 0));
    }
  }
  // the log: what took effect, in the order posted; one group index per communicator and group
  std::map<ncclComm *, long> gi;
  for (Op &o : ops) {
    World *w = o.c->w;
    if (!gi.count(o.c)) gi[o.c] = w->groups[o.c->rank]++;
    w->log[o.c->rank].push_back({o.kind == 's' ? "send" : o.kind == 'r' ? "recv" : "bcast", o.peer, o.bytes, gi[o.c]});
  }
  return ncclSuccess;
}

ncclResult_t run_group(std::vector<Op> &ops) {
  if (ops.empty()) return ncclSuccess;
  if (ncclResult_t e = check_overlaps(ops)) return e;
  std::unique_lock<std::mutex> lk(g_mu);
  for (Op &o : ops)
    if (!o.c->alive) return err(ncclInvalidArgument, "communicator destroyed: " + describe(o));
  const ncclResult_t e = run_locked(ops, lk);
  if (e != ncclSuccess) abandon(ops);
  return e;
}

ncclResult_t post(Op o, size_t count, ncclDataType_t type) {
  if (!o.c) return err(ncclInvalidArgument, "null communicator");
  const size_t ts = type_size(type);
  if (!ts) return err(ncclInvalidArgument, "unknown data type");
  o.bytes = count * ts;
  if (o.peer < 0 || o.peer >= o.c->w->nranks) return err(ncclInvalidArgument, "peer or root out of range: " + describe(o));
  if (o.bytes && ((o.kind != 'r' && !o.src && (o.kind == 's' || o.peer == o.c->rank)) || (o.kind != 's' && !o.dst)))
    return err(ncclInvalidArgument, "null buffer: " + describe(o));
  t_ops.push_back(o);
  if (t_depth > 0) return ncclSuccess;
  std::vector<Op> ops;
  ops.swap(t_ops);
  return run_group(ops);
}

uint64_t token_of(const void *id) {
  uint64_t t = 0;
  if (std::memcmp(id, kMagic, sizeof(kMagic)) == 0) std::memcpy(&t, (const char *)id + sizeof(kMagic), sizeof(t));
  return t;
}

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

ncclResult_t ncclGetUniqueId(ncclUniqueId *id) {  // touches no device
  if (!id) return err(ncclInvalidArgument, "null id");
  std::lock_guard<std::mutex> lk(g_mu);
  const uint64_t t = g_next_token++;
  g_worlds[t];
  std::memset(id, 0, sizeof(*id));
  std::memcpy(id->internal, kMagic, sizeof(kMagic));
  std::memcpy(id->internal + sizeof(kMagic), &t, sizeof(t));
  return ncclSuccess;
}

ncclResult_t ncclCommInitRank(ncclComm_t *comm, int nranks, ncclUniqueId id, int rank) {
  if (!comm || nranks < 1 || rank < 0 || rank >= nranks) return err(ncclInvalidArgument, "rank / nranks out of range");
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_worlds.find(token_of(id.internal));
  if (it == g_worlds.end()) return err(ncclInvalidArgument, "unique id not from ncclGetUniqueId");
  World &w = it->second;
  if (w.nranks == 0) {
    w.nranks = nranks;
    w.joined.assign(nranks, 0);
    w.ncoll.assign(nranks, 0);
    w.groups.assign(nranks, 0);
    w.log.resize(nranks);
  }
  if (w.nranks != nranks)
    return err(ncclInvalidArgument, "nranks " + std::to_string(nranks) + " joins a communicator of " + std::to_string(w.nranks));
  if (w.joined[rank]) return err(ncclInvalidArgument, "rank " + std::to_string(rank) + " joined twice");
  w.joined[rank] = 1;
  ++w.live;
  *comm = new ncclComm{&w, rank, true};
  return ncclSuccess;
}

ncclResult_t ncclCommDestroy(ncclComm_t comm) {
  if (!comm) return ncclSuccess;
  std::lock_guard<std::mutex> lk(g_mu);
  if (!comm->alive) return err(ncclInvalidArgument, "communicator destroyed twice");
  comm->alive = false;  // (the handle itself stays allocated, so that a late use is an error and not a stray read)
  World *w = comm->w;
  if (--w->live == 0) {
    for (hipEvent_t ev : w->events) (void)hipEventDestroy(ev);
    w->events.clear();
  }
  return ncclSuccess;
}

ncclResult_t ncclGroupStart() {
  ++t_depth;
  return ncclSuccess;
}

ncclResult_t ncclGroupEnd() {
  if (t_depth <= 0) return err(ncclInvalidUsage, "ncclGroupEnd without ncclGroupStart");
  if (--t_depth > 0) return ncclSuccess;
  std::vector<Op> ops;
  ops.swap(t_ops);
  return run_group(ops);
}

ncclResult_t ncclSend(const void *sendbuff, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t st) {
  return post(Op{'s', comm, sendbuff, nullptr, 0, peer, st}, count, type);
}

ncclResult_t ncclRecv(void *recvbuff, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t st) {
  return post(Op{'r', comm, nullptr, recvbuff, 0, peer, st}, count, type);
}

ncclResult_t ncclBroadcast(const void *sendbuff, void *recvbuff, size_t count, ncclDataType_t type, int root,
                           ncclComm_t comm, hipStream_t st) {
  return post(Op{'b', comm, sendbuff, recvbuff, 0, root, st}, count, type);
}

// the result's name and, after a failing call on this thread, what failed: the unmatched operation's kind, rank,
// peer or root and bytes
const char *ncclGetErrorString(ncclResult_t e) {
  static const char *names[] = {"success", "unhandled device error", "system error", "internal error",
                                "invalid argument", "invalid usage", "remote error", "in progress"};
  t_msg = (int)e >= 0 && (int)e < 8 ? names[(int)e] : "unknown result";
  if (e != ncclSuccess && !t_detail.empty()) t_msg += " (" + t_detail + ")";
  return t_msg.c_str();
}

// --- the test's side ---------------------------------------------------------------------------------------------
// the limit of every host-side wait, milliseconds; returns the previous one
long fake_rccl_set_wait_limit_ms(long ms) { return g_limit_ms.exchange(ms > 0 ? ms : 1); }

// rank's ordered record of the operations that took effect on the communicator of `id`, as JSON
// [[kind, peer or root, bytes, group index], ...] into buf (cap bytes, NUL included); returns the length needed
// (NUL excluded), or -1 for an unknown id or rank
long fake_rccl_log(const void *id, int rank, char *buf, long cap) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = id ? g_worlds.find(token_of(id)) : g_worlds.end();
  if (it == g_worlds.end() || rank < 0 || rank >= it->second.nranks) return -1;
  std::string s = "[";
  for (const LogEntry &e : it->second.log[rank]) {
    if (s.size() > 1) s += ",";
    s += std::string("[\"") + e.kind + "\"," + std::to_string(e.peer) + "," + std::to_string(e.bytes) + "," +
         std::to_string(e.group) + "]";
  }
  s += "]";
  if (buf && cap > (long)s.size()) std::memcpy(buf, s.c_str(), s.size() + 1);
  return (long)s.size();
}

}  // extern "C"
#pragma GCC visibility pop
