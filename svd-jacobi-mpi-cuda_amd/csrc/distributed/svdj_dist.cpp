// Device engine of the native distributed block one-sided Jacobi
// (svdj_dist.h): the handle, the half exchanges, their calibration, the
// watchdog and the solve.  It enqueues the plan of dist_plan.cpp (the file
// comment there describes a sweep) with RCCL + the HIP block kernels of
// libsvdj_hip.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <mutex>
#include <thread>
#include <tuple>
#include <vector>

#include "dist_plan.hpp"
#include "svdj_cpu.h"
#include "svdj_debug.h"
#include "svdj_dist.h"
#include "svdj_hip.h"

using namespace svdj::dist;

static_assert(sizeof(ncclUniqueId) == 128, "the id file (dist_plan.cpp) stores 128 id bytes");

namespace {

#define HIPC(x)                                                                    \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) return fail(-100, "%s:%d %s: %s", __FILE__, __LINE__, #x, \
                                      hipGetErrorString(e_));                      \
  } while (0)
#define NCCLC(x)                                                                   \
  do {                                                                             \
    ncclResult_t r_ = (x);                                                         \
    if (r_ != ncclSuccess) return fail(-200, "%s:%d %s: %s", __FILE__, __LINE__, #x, \
                                       ncclGetErrorString(r_));                    \
  } while (0)
#define SVDJC(x)                                                                   \
  do {                                                                             \
    int rc_ = (x);                                                                 \
    if (rc_ < 0) return fail(rc_, "%s:%d %s: %s", __FILE__, __LINE__, #x,           \
                             svdj_hip_last_error());                               \
  } while (0)

}  // namespace

extern "C" int svdj_dist_comm_init(int rank, int world, const char* id_path, double timeout_s,
                                   void** comm) {
  ncclUniqueId id;
  memset(&id, 0, sizeof(id));
  if (rank == 0) NCCLC(ncclGetUniqueId(&id));
  if (int r = svdj_dist_id_file(rank, id_path, timeout_s, &id, sizeof(id))) return r;
  ncclComm_t c;
  NCCLC(ncclCommInitRank(&c, world, id, rank));
  *comm = c;
  return 0;
}

extern "C" int svdj_dist_comm_destroy(void* comm) {
  if (comm) NCCLC(ncclCommDestroy((ncclComm_t)comm));
  return 0;
}

namespace {

// Fail-fast watchdog: a thread polls the RCCL async
// error and the time since the last finished sweep.  On a fault it takes the
// NCCL lock (the solve holds it around every group of RCCL calls, so the
// communicator is never freed under an enqueue), sets `fired` and calls
// ncclCommAbort, which releases RCCL kernels spinning on the dead peer so
// the streams drain; the solve returns -300 at its next check.  If the lock
// cannot be had for 5 s (an enqueue itself is stuck), the process exits 3.
struct Watchdog {
  std::atomic<bool> stop{false}, fired{false};
  std::mutex mu;  // held by the solve around RCCL calls
  std::atomic<long long> last_ns{0};
  char why[256] = {0};
  std::thread th;
  ~Watchdog() { join(); }
  static long long now_ns() {
    return std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch()).count();
  }
  void progress() { last_ns = now_ns(); }
  void start(ncclComm_t comm, double timeout_s, int rank) {
    progress();
    th = std::thread([this, comm, timeout_s, rank]() {
      while (!stop.load()) {
        std::this_thread::sleep_for(std::chrono::milliseconds(20));
        ncclResult_t ae = ncclSuccess;
        const ncclResult_t q = ncclCommGetAsyncError(comm, &ae);
        const double idle = (now_ns() - last_ns.load()) * 1e-9;
        if (q != ncclSuccess || (ae != ncclSuccess && ae != ncclInProgress)) {
          snprintf(why, sizeof(why), "rank %d: RCCL async error: %s", rank,
                   ncclGetErrorString(q != ncclSuccess ? q : ae));
        } else if (idle > timeout_s) {
          snprintf(why, sizeof(why), "rank %d: no sweep finished for %.0f s (peer dead or hung)",
                   rank, idle);
        } else {
          continue;
        }
        fprintf(stderr, "[svdj_dist watchdog] %s: aborting the communicator\n", why);
        fflush(stderr);
        const long long t_lock = now_ns();
        while (!mu.try_lock()) {
          if ((now_ns() - t_lock) * 1e-9 > 5.0) {
            fprintf(stderr, "[svdj_dist watchdog] rank %d: RCCL call stuck, exiting\n", rank);
            fflush(stderr);
            _exit(3);
          }
          std::this_thread::sleep_for(std::chrono::milliseconds(5));
        }
        fired = true;
        (void)ncclCommAbort(comm);
        mu.unlock();
        return;
      }
    });
  }
  void join() {
    stop = true;
    if (th.joinable()) th.join();
  }
};

}  // namespace

struct svdj_dist_handle_t {
  int rank, world, dtype, W, m_pad, n_v, B, k, hk, hB, has_v, timing;
  bool spread = false;           // exchanges relayed over all links (parallel/spread.py)
  int io = 0;                    // resolved EVD order of the cross steps (0 cyclic, 1 bip, 2 cross)
  void* relay[2] = {nullptr, nullptr};  // A / V relay chunks, one row per source rank
  size_t relay_n[2] = {0, 0};           // elements per row
  ncclComm_t comm;
  hipStream_t st[2], sc;
  bool own_sc = false;
  size_t es, wsb;
  void* ws[2] = {nullptr, nullptr};
  uint32_t* metric = nullptr;
  bool quad = false;    // quad steps (two cross steps fused) in every template
  bool merged = false;  // one GPU: each parallel task pair issued as one launch of twice the pairs
  PairLists pl;         // host pairs and modes of the templates, merged lists
  int32_t* pairs_pool = nullptr;      // device pairs of every template in every placement
  int32_t* dev[kTemplates][6][6] = {};  // [template][buffer of hv[0]][buffer of hv[1]] -> into the pool
  int32_t* merged_pairs = nullptr;    // [rr0+rr1 | T00+T11 | T01+T10], device
  double calib_ms[2] = {0, 0};  // exchange calibration: direct, spread (0: not run)
  std::vector<Item> items;
  std::vector<Group> groups;
  // per item: end event (task) / arrival (send); timing: start (task) / issue
  // (send), consumer-ready events (two per task); plus sweep start and join
  std::vector<hipEvent_t> ev, ev_start, ev_ready;
  hipEvent_t ev_t0 = nullptr, ev_join = nullptr;
  Layout L;
};

namespace {

// Device copies of the plan's pair lists (dist_plan.cpp pair_lists): one per
// placement of each template's halves and, on one GPU, the merged lists.
int build_templates(svdj_dist_handle_t* h) {
  h->pl = pair_lists(h->k, h->quad, h->merged, svdj_cross_step_mode(h->io));
  std::vector<int32_t> pool;
  std::vector<std::tuple<int, int, int, size_t>> where;
  for (int t = 0; t < kTemplates; ++t)
    for (auto [ba, bb] : placements(h->pl.t[t].hv, h->world)) {
      where.emplace_back(t, ba, bb, pool.size());
      place_pairs(h->pl.t[t], h->k, ba, bb, pool);
    }
  HIPC(hipMalloc((void**)&h->pairs_pool, pool.size() * sizeof(int32_t)));
  HIPC(hipMemcpy(h->pairs_pool, pool.data(), pool.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  for (auto [t, ba, bb, at] : where) h->dev[t][ba][bb] = h->pairs_pool + at;
  if (h->merged) {
    const std::vector<int32_t>& mp = h->pl.merged_pairs;
    HIPC(hipMalloc((void**)&h->merged_pairs, mp.size() * sizeof(int32_t)));
    HIPC(hipMemcpy(h->merged_pairs, mp.data(), mp.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  return 0;
}

void handle_free(svdj_dist_handle_t* h) {
  if (!h) return;
  for (auto* v : {&h->ev, &h->ev_start, &h->ev_ready})
    for (auto& e : *v)
      if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : {h->ev_t0, h->ev_join})
    if (e) (void)hipEventDestroy(e);
  if (h->own_sc && h->sc) (void)hipStreamDestroy(h->sc);
  (void)hipFree(h->pairs_pool);
  (void)hipFree(h->merged_pairs);
  (void)hipFree(h->relay[0]);
  (void)hipFree(h->relay[1]);
  (void)hipFree(h->ws[0]);
  (void)hipFree(h->ws[1]);
  (void)hipFree(h->metric);
  delete h;
}

// One half exchange of tournament round `round` on stream sc (grouped RCCL):
// each message goes to send_to and arrives from recv_from, directly, or
// (spread, a message with a relay buffer) cut into P-1 near-equal chunks --
// chunk 0 direct, chunk j >= 1 via the j-th rank not in {sender, receiver}
// -- in two grouped phases (parallel/spread.py).  The data that arrives is
// the same bit for bit.
struct XMsg {
  char *out, *in;
  size_t n;
  char* relay;  // non-null: relayed (spread)
  size_t relay_n;
};
int exchange_ops(const Tour& tour, int round, int g, const XMsg* msgs, int nm, bool spread,
                 ncclDataType_t nt, size_t es, ncclComm_t comm, hipStream_t sc) {
  const int P = tour.P, dst = tour.to(round, g), src = tour.from(round, g);
  auto piece = [&](size_t n, int j, size_t& a, size_t& len) {
    const size_t base = n / (P - 1), rem = n % (P - 1);
    a = j * base + ((size_t)j < rem ? (size_t)j : rem);
    len = base + ((size_t)j < rem ? 1 : 0);
  };
  auto relay_index = [&](int s, int d, int q) {
    int j = 0;
    for (int x = 0; x < P; ++x) {
      if (x == s || x == d) continue;
      ++j;
      if (x == q) return j;
    }
    return -1;
  };
  size_t a0, ln;
  NCCLC(ncclGroupStart());  // direct messages / phase 1
  for (int i = 0; i < nm; ++i) {
    const XMsg& M = msgs[i];
    if (!spread || !M.relay) {
      NCCLC(ncclSend(M.out, M.n, nt, dst, comm, sc));
      NCCLC(ncclRecv(M.in, M.n, nt, src, comm, sc));
      continue;
    }
    piece(M.n, 0, a0, ln);
    NCCLC(ncclSend(M.out + a0 * es, ln, nt, dst, comm, sc));
    for (int q = 0, j = 0; q < P; ++q) {
      if (q == g || q == dst) continue;
      piece(M.n, ++j, a0, ln);
      NCCLC(ncclSend(M.out + a0 * es, ln, nt, q, comm, sc));
    }
    piece(M.n, 0, a0, ln);
    NCCLC(ncclRecv(M.in + a0 * es, ln, nt, src, comm, sc));
    for (int s = 0; s < P; ++s) {  // sources this rank relays for
      if (s == g || s == src) continue;
      piece(M.n, relay_index(s, tour.to(round, s), g), a0, ln);
      NCCLC(ncclRecv(M.relay + (size_t)s * M.relay_n * es, ln, nt, s, comm, sc));
    }
  }
  NCCLC(ncclGroupEnd());
  if (spread) {  // phase 2: forward the relayed chunks, receive ours
    NCCLC(ncclGroupStart());
    for (int i = 0; i < nm; ++i) {
      const XMsg& M = msgs[i];
      if (!M.relay) continue;
      for (int s = 0; s < P; ++s) {
        if (s == g || s == src) continue;
        const int d = tour.to(round, s);
        piece(M.n, relay_index(s, d, g), a0, ln);
        NCCLC(ncclSend(M.relay + (size_t)s * M.relay_n * es, ln, nt, d, comm, sc));
      }
      for (int q = 0, j = 0; q < P; ++q) {
        if (q == src || q == g) continue;
        piece(M.n, ++j, a0, ln);
        NCCLC(ncclRecv(M.in + a0 * es, ln, nt, q, comm, sc));
      }
    }
    NCCLC(ncclGroupEnd());
  }
  return 0;
}

// Wait for stream s without blocking forever.  Handle creation runs before
// the solve's watchdog exists, so its collectives are polled here: an RCCL
// async error or timeout_s without completion aborts the communicator (the
// RCCL kernels spinning on a dead peer are released and the stream drains)
// and returns -300, as a watchdog abort in svdj_dist_solve does.
int poll_stream(hipStream_t s, ncclComm_t comm, double timeout_s) {
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    const hipError_t q = hipStreamQuery(s);
    if (q == hipSuccess) return 0;
    if (q != hipErrorNotReady) return fail(-100, "stream error: %s", hipGetErrorString(q));
    ncclResult_t ae = ncclSuccess;
    const ncclResult_t r = ncclCommGetAsyncError(comm, &ae);
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (r != ncclSuccess || (ae != ncclSuccess && ae != ncclInProgress) || el > timeout_s) {
      (void)ncclCommAbort(comm);
      (void)hipStreamSynchronize(s);
      return fail(-300, "handle creation: %s; communicator aborted",
                  el > timeout_s ? "collective timed out" : "RCCL async error");
    }
    std::this_thread::sleep_for(std::chrono::microseconds(50));
  }
}

// Exchange calibration (pipeline.calibrate_exchange, ADVICE r3 / VERDICT r4):
// at handle creation, from 4 ranks with exchange auto, one half exchange of
// the first tournament round is timed both ways on this job's links (real
// half-buffer sizes of A, the norms and V; one warm-up, the best of 3; every
// timing the max over ranks), and spread is kept only if it is >= 10 %
// faster.  Every rank takes the same decision (the times are all-reduced).
int calibrate_exchange(svdj_dist_handle_t* h, double timeout_s) {
  const int P = h->world, g = h->rank;
  Tour tour(P);
  const size_t es = h->es;
  const ncclDataType_t nt = h->dtype == 1 ? ncclFloat64 : ncclFloat32;
  const size_t n[3] = {(size_t)h->hB * h->m_pad, (size_t)h->hB, h->has_v ? (size_t)h->hB * h->n_v : 0};
  char* buf[3][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
  double* dt = nullptr;
  int rc = 0;
  for (int i = 0; i < 3 && !rc; ++i)
    for (int j = 0; j < 2 && !rc && n[i]; ++j)
      if (hipMalloc((void**)&buf[i][j], n[i] * es) != hipSuccess || hipMemset(buf[i][j], 0, n[i] * es) != hipSuccess)
        rc = fail(-100, "calibration buffers: hipMalloc failed");
  if (!rc && hipMalloc((void**)&dt, sizeof(double)) != hipSuccess) rc = fail(-100, "hipMalloc failed");
  double best[2] = {1e30, 1e30};
  for (int v = 0; v < 2 && !rc; ++v) {
    const bool spread = v == 1;
    XMsg msgs[3];
    int nm = 0;
    msgs[nm++] = {buf[0][0], buf[0][1], n[0], spread ? (char*)h->relay[0] : nullptr, h->relay_n[0]};
    msgs[nm++] = {buf[1][0], buf[1][1], n[1], nullptr, 0};
    if (n[2]) msgs[nm++] = {buf[2][0], buf[2][1], n[2], spread ? (char*)h->relay[1] : nullptr, h->relay_n[1]};
    for (int it = 0; it < 4 && !rc; ++it) {
      // line the ranks up (a tiny all-reduce), then time one exchange
      if (ncclAllReduce(dt, dt, 1, ncclFloat64, ncclMax, h->comm, h->sc) != ncclSuccess) {
        rc = fail(-200, "calibration barrier failed");
        break;
      }
      if ((rc = poll_stream(h->sc, h->comm, timeout_s))) break;
      const auto t0 = std::chrono::steady_clock::now();
      if ((rc = exchange_ops(tour, 1, g, msgs, nm, spread, nt, es, h->comm, h->sc))) break;
      if ((rc = poll_stream(h->sc, h->comm, timeout_s))) break;
      double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
      if (hipMemcpy(dt, &t, sizeof(t), hipMemcpyHostToDevice) != hipSuccess ||
          ncclAllReduce(dt, dt, 1, ncclFloat64, ncclMax, h->comm, h->sc) != ncclSuccess) {
        rc = fail(-200, "calibration max over ranks failed");
        break;
      }
      if ((rc = poll_stream(h->sc, h->comm, timeout_s))) break;
      if (hipMemcpy(&t, dt, sizeof(t), hipMemcpyDeviceToHost) != hipSuccess) {
        rc = fail(-100, "calibration copy failed");
        break;
      }
      if (it) best[v] = std::min(best[v], t);
    }
  }
  for (auto& b : buf)
    for (char* x : b) (void)hipFree(x);
  (void)hipFree(dt);
  if (rc) return rc;
  h->calib_ms[0] = best[0] * 1e3;
  h->calib_ms[1] = best[1] * 1e3;
  h->spread = best[1] < 0.9 * best[0];
  if (!h->spread)
    for (void*& r : h->relay) {
      (void)hipFree(r);
      r = nullptr;
    }
  return 0;
}

// ---- svdj_dist_handle_create, step by step; each returns 0 or the failure.

// The problem's fields, the EVD order, the issue rules and the exchange.
int resolve_rules(svdj_dist_handle_t* h, const svdj_dist_problem* p) {
  const int W = p->W, B = p->B;
  h->rank = p->rank, h->world = p->world, h->dtype = p->dtype, h->W = W, h->m_pad = p->m_pad;
  h->n_v = p->n_v, h->B = B, h->k = B / W, h->hk = h->k / 2, h->hB = h->hk * W;
  h->has_v = p->Vt != nullptr, h->timing = p->comm_timing != 0;
  h->comm = (ncclComm_t)p->comm;
  h->st[0] = (hipStream_t)p->stream_a;
  h->st[1] = (hipStream_t)p->stream_b;
  h->sc = (hipStream_t)p->stream_comm;
  h->es = p->dtype == 1 ? 8 : 4;
  // auto: by the pairs of a cross step (half super-blocks)
  h->io = p->inner_order == SVDJ_INNER_AUTO ? svdj_choose_inner_order(p->dtype, W, h->hk)
                                            : p->inner_order;
  h->spread = h->world > 2 && (p->exchange == 2 || (p->exchange == 0 && h->world >= 4));
  // quad steps from 32 pairs per chain step on any number of GPUs, merged
  // issue on one GPU from 64 pairs (32 with quad steps) -- the Python
  // engine's rules: models/block.py choose_quad, choose_merged
  int quad = 0, merged = 0;
  const int rc = svdj_dist_issue_rules(p->world, p->dtype, W, p->mma, h->k, p->m_pad, p->quad,
                                       &quad, &merged);
  h->quad = quad != 0;
  h->merged = merged != 0;
  if (rc < 0) return rc;
  if (p->exchange < 0 || p->exchange > 2)
    return fail(-2, "exchange %d (0 auto, 1 direct, 2 spread)", p->exchange);
  return 0;
}

int alloc_workspaces(svdj_dist_handle_t* h) {
  h->wsb = svdj_block_workspace_bytes(h->dtype, h->W, h->merged ? h->k : h->k / 2, h->m_pad,
                                      h->quad ? 1 : 0);
  for (int c = 0; c < 2; ++c)
    if (hipMalloc(&h->ws[c], h->wsb) != hipSuccess) return fail(-100, "hipMalloc(ws %zu) failed", h->wsb);
  if (hipMalloc((void**)&h->metric, SVDJ_METRIC_WORDS * sizeof(uint32_t)) != hipSuccess)
    return fail(-100, "hipMalloc(metric) failed");
  return 0;
}

int alloc_relay(svdj_dist_handle_t* h) {
  if (!h->spread) return 0;  // chunk rows: ceil(message / (P - 1)) elements
  const size_t msg[2] = {(size_t)h->hB * h->m_pad, h->has_v ? (size_t)h->hB * h->n_v : 0};
  for (int i = 0; i < 2; ++i) {
    h->relay_n[i] = (msg[i] + h->world - 2) / (h->world - 1);
    if (msg[i] && hipMalloc(&h->relay[i], h->relay_n[i] * h->world * h->es) != hipSuccess)
      return fail(-100, "hipMalloc(relay %zu) failed", h->relay_n[i] * h->world * h->es);
  }
  return 0;
}

int make_comm_stream(svdj_dist_handle_t* h) {
  if (h->sc || h->world <= 1) return 0;
  if (hipStreamCreateWithFlags(&h->sc, hipStreamNonBlocking) != hipSuccess)
    return fail(-100, "comm stream creation failed");
  h->own_sc = true;
  return 0;
}

// Measured exchange choice: a collective, so first a go/no-go over ALL
// ranks (max of the local failure flags; a rank that failed above, rc != 0,
// still takes part), then every rank calibrates or every rank gives up -- a
// rank that skipped calibration alone would leave its peers blocked in it.
int go_and_calibrate(svdj_dist_handle_t* h, double tmo, int rc) {
  int32_t* flag = nullptr;
  int32_t any = rc ? 1 : 0;
  if (hipMalloc((void**)&flag, sizeof(int32_t)) != hipSuccess ||
      hipMemcpy(flag, &any, sizeof(any), hipMemcpyHostToDevice) != hipSuccess) {
    rc = rc ? rc : fail(-100, "go/no-go flag: hipMalloc failed");
  } else if (ncclAllReduce(flag, flag, 1, ncclInt32, ncclMax, h->comm, h->sc) != ncclSuccess) {
    rc = rc ? rc : fail(-200, "go/no-go all-reduce failed");
  } else if (int r = poll_stream(h->sc, h->comm, tmo)) {
    rc = rc ? rc : r;
  } else if (hipMemcpy(&any, flag, sizeof(any), hipMemcpyDeviceToHost) != hipSuccess) {
    rc = rc ? rc : fail(-100, "go/no-go flag copy failed");
  } else if (any && !rc) {
    rc = fail(-2, "handle creation failed on another rank: exchange calibration skipped");
  }
  (void)hipFree(flag);
  return rc ? rc : calibrate_exchange(h, tmo);
}

}  // namespace

extern "C" int svdj_dist_handle_create(const svdj_dist_problem* p, void** out) {
  *out = nullptr;
  if (p->W <= 0 || p->B % p->W || (p->B / p->W) < 2 || (p->B / p->W) % 2)
    return fail(-2, "B=%d must hold an even number of W=%d blocks", p->B, p->W);
  if (p->stream_a == p->stream_b) return fail(-2, "two distinct streams needed");
  auto* h = new svdj_dist_handle_t();
  int rc = resolve_rules(h, p);
  if (!rc) rc = build_templates(h);
  if (!rc) rc = alloc_workspaces(h);
  if (!rc) rc = alloc_relay(h);
  if (!rc) rc = make_comm_stream(h);
  if (h->world >= 4 && p->exchange == 0 && h->sc)
    rc = go_and_calibrate(h, p->timeout_s > 0 ? p->timeout_s : 600.0, rc);
  if (rc) {
    handle_free(h);
    return rc;
  }
  *out = h;
  return 0;
}

extern "C" int svdj_dist_handle_destroy(void* handle) {
  handle_free((svdj_dist_handle_t*)handle);
  return 0;
}

namespace {

// The issue plan of this rank and its events (kept in the handle after the
// first solve).
int ensure_plan(svdj_dist_handle_t* h, const Tour& tour) {
  if (!h->items.empty()) return 0;
  h->items = sweep_items(tour, h->rank);
  h->groups = issue_groups(h->items);
  const unsigned flags = h->timing ? 0 : hipEventDisableTiming;
  h->ev.assign(h->items.size(), nullptr);
  for (auto& e : h->ev) HIPC(hipEventCreateWithFlags(&e, flags));
  if (h->timing) {
    h->ev_start.assign(h->items.size(), nullptr);
    h->ev_ready.assign(2 * h->items.size(), nullptr);
    for (auto* v : {&h->ev_start, &h->ev_ready})
      for (auto& e : *v) HIPC(hipEventCreateWithFlags(&e, 0));
    HIPC(hipEventCreateWithFlags(&h->ev_t0, 0));
  }
  HIPC(hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming));
  return 0;
}

// State of one svdj_dist_solve call.  Stream st[0] carries everything that
// is not a task of chain 1 or an exchange (stream sc).
struct Solve {
  using EventSpans = std::vector<std::pair<hipEvent_t, hipEvent_t>>;
  svdj_dist_handle_t* h;
  svdj_dist_problem* p;
  Tour tour;
  Watchdog wd;
  std::vector<int32_t> phys;  // placement of every GPU's slots (all ranks simulate the whole table)
  int mma_sweep;              // the apply's mode, | SVDJ_STEPS_GRAM2 for a 2-part quad Gram
  // of the sweep being issued
  std::vector<hipEvent_t> last[4];  // task events on each half since its last exchange
  hipEvent_t pending[4] = {};       // arrived, not yet waited
  int halves_sent = 0;
  EventSpans sp_busy, sp_wait, sp_span;
  // of the whole solve
  Spans busy, waits;
  double comm_ms = 0, sweep_base_ms = 0;
  long long n_exch = 0, n_bytes = 0;

  Solve(svdj_dist_handle_t* h_, svdj_dist_problem* p_)
      : h(h_), p(p_), tour(h_->world), phys(2 * h_->world), mma_sweep(p_->mma) {}

  char* buf_ptr(void* base, size_t ld, int b) const {
    return (char*)base + (size_t)b * h->hB * ld * h->es;
  }
  // Wait for stream st[0] without blocking forever: poll, and give up when
  // the watchdog fired (a dead peer leaves RCCL kernels spinning; the abort
  // releases them and the stream drains).
  int wait_sa() {
    for (;;) {
      const hipError_t q = hipStreamQuery(h->st[0]);
      if (q == hipSuccess) return 0;
      if (q != hipErrorNotReady) return fail(-100, "stream error: %s", hipGetErrorString(q));
      if (wd.fired.load()) return fail(-300, "%s", wd.why);
      std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
  }
  int block_steps(const int32_t* pairs, int npairs, int steps, const int32_t* modes, int chain,
                  int flags, hipStream_t s) {
    SVDJC(svdj_block_steps(h->dtype, h->W, h->m_pad, p->At, h->m_pad, p->Vt, h->n_v, h->n_v, p->D,
                           pairs, npairs, steps, modes, p->tol, p->tol_mode, 1, h->ws[chain], h->wsb,
                           h->metric, flags, s));
    return 0;
  }
  // One GPU: three merged launches on one stream, nothing to wait for.
  int merged_sweep() {
    const PairLists& pl = h->pl;
    for (int m = 0; m < 3; ++m)
      if (int r = block_steps(h->merged_pairs + pl.merged_off[m], pl.merged_np[m], pl.merged_steps[m],
                              pl.merged_modes[m].data(), 0, mma_sweep, h->st[0]))
        return r;
    return 0;
  }
  // One half of slot a.slot to send_to, its replacement from recv_from.
  int issue_send(const Item& a, int ia) {
    hipStream_t sc = h->sc;
    Layout& L = h->L;
    const int hB = h->hB;
    const size_t es = h->es;
    const int key = a.slot * 2 + a.half;
    const int out_b = L.loc[a.slot][a.half], in_b = L.spare[a.half];
    for (hipEvent_t e : last[key]) HIPC(hipStreamWaitEvent(sc, e, 0));
    last[key].clear();
    if (h->timing) HIPC(hipEventRecord(h->ev_start[ia], sc));
    std::unique_lock<std::mutex> lk(wd.mu);
    if (wd.fired.load()) return fail(-300, "%s", wd.why);
    // messages in the order of pipeline.py: A half, norms, V half
    XMsg msgs[3];
    int nm = 0;
    msgs[nm++] = {buf_ptr(p->At, h->m_pad, out_b), buf_ptr(p->At, h->m_pad, in_b),
                  (size_t)hB * h->m_pad, h->spread ? (char*)h->relay[0] : nullptr, h->relay_n[0]};
    msgs[nm++] = {(char*)p->D + (size_t)out_b * hB * es, (char*)p->D + (size_t)in_b * hB * es,
                  (size_t)hB, nullptr, 0};
    if (p->Vt)
      msgs[nm++] = {buf_ptr(p->Vt, h->n_v, out_b), buf_ptr(p->Vt, h->n_v, in_b),
                    (size_t)hB * h->n_v, h->spread ? (char*)h->relay[1] : nullptr, h->relay_n[1]};
    ++n_exch;
    for (int i = 0; i < nm; ++i) n_bytes += (long long)msgs[i].n * (long long)es;
    const ncclDataType_t nt = h->dtype == 1 ? ncclFloat64 : ncclFloat32;
    if (int r = exchange_ops(tour, a.round, h->rank, msgs, nm, h->spread, nt, es, h->comm, sc))
      return r;
    lk.unlock();
    // received in place: from here on (issue order) the half lives in in_b;
    // in_b's last readers were waited for by the exchange that freed it
    L.loc[a.slot][a.half] = in_b;
    L.spare[a.half] = out_b;
    hipEvent_t arrived = h->ev[ia];
    HIPC(hipEventRecord(arrived, sc));
    if (h->timing) sp_span.push_back({h->ev_start[ia], arrived});
    pending[key] = arrived;
    if (++halves_sent % 2 == 0) {  // both halves of round a.round issued: new placement
      std::vector<int32_t> old = phys;
      for (int r = 0; r < tour.P; ++r) {
        const int sh = tour.from(a.round, r);
        phys[2 * r + tour.x(a.round, r)] = old[2 * sh + tour.x(a.round, sh)];
      }
    }
    return 0;
  }
  // One chain, or two issued independently: waits of both, launches, records.
  int issue_tasks(const Group& gr) {
    const int n_t = gr.b < 0 ? 1 : 2;
    const int idx[2] = {gr.a, gr.b};
    for (int q = 0; q < n_t; ++q) {
      const Item& x = h->items[idx[q]];
      hipStream_t s = h->st[x.stream];
      int nready = 0;
      for (int hv : x.hv) {
        for (hipEvent_t e : last[hv]) HIPC(hipStreamWaitEvent(s, e, 0));
        if (pending[hv]) {
          if (h->timing) {
            hipEvent_t r = h->ev_ready[2 * idx[q] + nready++];
            HIPC(hipEventRecord(r, s));
            sp_wait.push_back({r, pending[hv]});
          }
          HIPC(hipStreamWaitEvent(s, pending[hv], 0));
          pending[hv] = nullptr;
        }
      }
      if (h->timing) HIPC(hipEventRecord(h->ev_start[idx[q]], s));
    }
    for (int q = 0; q < n_t; ++q) {
      const Item& x = h->items[idx[q]];
      const Template& t = h->pl.t[x.tmpl];
      const int ba = h->L.loc[t.hv[0] / 2][t.hv[0] % 2], bb = h->L.loc[t.hv[1] / 2][t.hv[1] % 2];
      if (int r = block_steps(h->dev[x.tmpl][ba][bb], t.npairs, t.steps, t.modes.data(), x.stream,
                              mma_sweep | (h->quad ? SVDJ_STEPS_SHARED_GPU : 0), h->st[x.stream]))
        return r;
    }
    for (int q = 0; q < n_t; ++q) {
      const Item& x = h->items[idx[q]];
      hipEvent_t e = h->ev[idx[q]];
      HIPC(hipEventRecord(e, h->st[x.stream]));
      if (h->timing) sp_busy.push_back({h->ev_start[idx[q]], e});
      for (int hv : x.hv) last[hv].push_back(e);
    }
    return 0;
  }
  // End of a sweep: both other streams join st[0]; with timing, this sweep's
  // events are resolved now.
  int join_and_time() {
    hipStream_t sa = h->st[0];
    HIPC(hipEventRecord(h->ev_join, h->st[1]));
    HIPC(hipStreamWaitEvent(sa, h->ev_join, 0));
    if (h->sc) {
      HIPC(hipEventRecord(h->ev_join, h->sc));
      HIPC(hipStreamWaitEvent(sa, h->ev_join, 0));
    }
    if (!h->timing) return 0;
    if (int r = wait_sa()) return r;
    auto t = [&](hipEvent_t e) {
      float ms = 0;
      (void)hipEventElapsedTime(&ms, h->ev_t0, e);
      return (double)ms + sweep_base_ms;
    };
    for (auto& x : sp_busy) busy.push_back({t(x.first), t(x.second)});
    for (auto& x : sp_wait) waits.push_back({t(x.first), t(x.second)});
    for (auto& x : sp_span) {
      float ms = 0;
      (void)hipEventElapsedTime(&ms, x.first, x.second);
      comm_ms += ms;
    }
    sweep_base_ms += 1e7;  // sweeps never overlap: keep their intervals apart
    return 0;
  }
  // One sweep: every dependency is an event; the host never waits.
  int sweep() {
    hipStream_t sa = h->st[0];
    if (svdj_reset_metric(h->metric, sa) != 0) return fail(-100, "metric reset failed");
    if (h->merged) return merged_sweep();
    for (int v = 0; v < 4; ++v) last[v].clear(), pending[v] = nullptr;
    halves_sent = 0;
    sp_busy.clear(), sp_wait.clear(), sp_span.clear();
    if (h->timing) HIPC(hipEventRecord(h->ev_t0, sa));
    HIPC(hipEventRecord(h->ev_join, sa));
    HIPC(hipStreamWaitEvent(h->st[1], h->ev_join, 0));
    if (h->sc) HIPC(hipStreamWaitEvent(h->sc, h->ev_join, 0));
    for (const Group& gr : h->groups) {
      const Item& a = h->items[gr.a];
      if (int r = a.send ? issue_send(a, gr.a) : issue_tasks(gr)) return r;
    }
    return join_and_time();
  }
  // Stop test (svdj_stop.h): global max convergence value and largest applied
  // |sin| (positive floats order as uint32), total rotated pairs -> hm.
  int reduce(uint32_t hm[6]) {
    hipStream_t sa = h->st[0];
    {
      std::lock_guard<std::mutex> lk(wd.mu);
      if (wd.fired.load()) return fail(-300, "%s", wd.why);
      if (h->world > 1) {  // one GPU (comm may be NULL): the local words are the global ones
        NCCLC(ncclAllReduce(h->metric, h->metric, 1, ncclUint32, ncclMax, h->comm, sa));
        NCCLC(ncclAllReduce(h->metric + 1, h->metric + 1, 1, ncclUint32, ncclSum, h->comm, sa));
        NCCLC(ncclAllReduce(h->metric + 4, h->metric + 4, 1, ncclUint32, ncclMax, h->comm, sa));
        NCCLC(ncclAllReduce(h->metric + 5, h->metric + 5, 1, ncclUint32, ncclSum, h->comm, sa));
      }
    }
    HIPC(hipMemcpyAsync(hm, h->metric, 6 * sizeof(uint32_t), hipMemcpyDeviceToHost, sa));
    return wait_sa();
  }
  // Halves back home (rows [sB, (s+1)B) = slot s).
  int canonicalise() {
    hipStream_t sa = h->st[0];
    const size_t hB = h->hB, es = h->es;
    for (auto& mv : moves_to_canonical(h->L)) {
      const size_t src = (size_t)mv.first, dst = (size_t)mv.second;
      if (hipMemcpyAsync(buf_ptr(p->At, h->m_pad, dst), buf_ptr(p->At, h->m_pad, src),
                         hB * h->m_pad * es, hipMemcpyDeviceToDevice, sa) != hipSuccess ||
          (p->Vt && hipMemcpyAsync(buf_ptr(p->Vt, h->n_v, dst), buf_ptr(p->Vt, h->n_v, src),
                                   hB * h->n_v * es, hipMemcpyDeviceToDevice, sa) != hipSuccess) ||
          hipMemcpyAsync((char*)p->D + dst * hB * es, (char*)p->D + src * hB * es, hB * es,
                         hipMemcpyDeviceToDevice, sa) != hipSuccess)
        return fail(-100, "canonicalise copy failed");
    }
    return 0;
  }
};

}  // namespace

extern "C" int svdj_dist_solve(svdj_dist_problem* p, void* sigma) {
  svdj_dist_handle_t* h = (svdj_dist_handle_t*)p->handle;
  bool own = false;
  if (!h) {
    void* hh = nullptr;
    if (int r = svdj_dist_handle_create(p, &hh)) return r;
    h = (svdj_dist_handle_t*)hh;
    own = true;
  }
  struct Own {
    svdj_dist_handle_t* h;
    bool own;
    ~Own() {
      if (own) handle_free(h);
    }
  } own_guard{h, own};
  if (h->rank != p->rank || h->world != p->world || h->dtype != p->dtype || h->W != p->W ||
      h->m_pad != p->m_pad || h->n_v != p->n_v || h->B != p->B || h->has_v != (p->Vt != nullptr) ||
      h->comm != (ncclComm_t)p->comm)
    return fail(-2, "handle does not match the problem geometry");
  const int P = h->world, g = h->rank;
  hipStream_t sa = h->st[0];
  Solve s(h, p);
  if (int r = ensure_plan(h, s.tour)) return r;
  h->L = Layout();
  if (P == 1) h->L.spare[0] = h->L.spare[1] = -1;
  for (int r = 0; r < P; ++r) {
    s.phys[2 * r] = s.tour.h(0, r, 0);
    s.phys[2 * r + 1] = s.tour.h(0, r, 1);
  }
  if (p->held[0] != s.phys[2 * g] || p->held[1] != s.phys[2 * g + 1])
    return fail(-2, "rank %d holds (%d, %d), the tournament starts from (%d, %d)", g, p->held[0],
                p->held[1], s.phys[2 * g], s.phys[2 * g + 1]);

  Watchdog& wd = s.wd;
  if (P > 1) wd.start(h->comm, p->timeout_s > 0 ? p->timeout_s : 600.0, g);
  int rc = 0;
  p->sweeps = 0;
  p->converged = 0;
  // negligible-column floor of the block EVDs (block.hip needs_rotation),
  // relative to the largest squared column norm: local value, then the max
  // over ranks (the floor is monotone in that norm)
  if (svdj_set_norm_floor_scaled(h->dtype, h->m_pad, p->D, 2 * p->B, h->metric, sa) < 0)
    return fail(-100, "norm floor: %s", svdj_hip_last_error());
  if (P > 1 &&
      ncclAllReduce(h->metric + 2, h->metric + 2, 1, ncclFloat64, ncclMax, h->comm, sa) != ncclSuccess)
    return fail(-200, "norm floor all-reduce failed");
  p->inner_order_used = h->io;
  p->exchange_used = P > 1 ? (h->spread ? 2 : 1) : 0;
  p->quad_used = h->quad ? 1 : 0;
  p->merged_used = h->merged ? 1 : 0;
  p->calib_direct_ms = h->calib_ms[0];
  p->calib_spread_ms = h->calib_ms[1];
  const auto t_solve = std::chrono::steady_clock::now();
  // Quad Gram precision per sweep (distributed.py next_gram_parts, the same rule):
  // 2 bf16 parts (SVDJ_STEPS_GRAM2) while the previous sweep
  // rotated every pair; SVDJ_DEBUG gram2=0/1 forces it off / on (A/B).
  const long long nbt = 2LL * P * h->k, all_pairs = nbt * (nbt - 1) / 2;
  const int gram2 = svdj_debug_knob("gram2", -1);
  bool prev_all = true;
  for (int sw = 0; sw < p->max_sweeps && !rc; ++sw) {
    s.mma_sweep =
        p->mma | ((h->quad && (gram2 < 0 ? prev_all : gram2 == 1)) ? SVDJ_STEPS_GRAM2 : 0);
    if ((rc = s.sweep())) break;
    uint32_t hm[6] = {0, 0, 0, 0, 0, 0};
    if ((rc = s.reduce(hm))) break;
    if (wd.fired.load()) {
      rc = fail(-300, "%s", wd.why);
      break;
    }
    wd.progress();
    float mx, ms;
    memcpy(&mx, &hm[0], sizeof(float));
    memcpy(&ms, &hm[4], sizeof(float));
    prev_all = (long long)hm[1] >= all_pairs;
    if (p->hist) p->hist[sw] = mx;
    p->sweeps = sw + 1;
    if (p->progress && g == 0) {
      const double el =
          std::chrono::duration<double>(std::chrono::steady_clock::now() - t_solve).count();
      fprintf(stderr,
              "[svdj_dist] sweep %d: off %.3e, eff sin %.3e, rotated pairs %u, rotations %u, %.2f s\n",
              sw + 1, (double)mx, (double)ms, hm[1], hm[5], el);
      fflush(stderr);
    }
    if (p->fault_rank == g && p->fault_sweep == sw + 1) {
      fprintf(stderr, "[svdj_dist] fault injection: rank %d exits after sweep %d\n", g, sw + 1);
      fflush(stderr);
      _exit(17);
    }
    const int conv =
        svdj_sweep_converged_inline(mx, ms, hm[1], hm[5], p->tol, p->tol_mode, p->stop_rule);
    if (conv) {
      p->converged = conv;
      break;
    }
  }
  if (!rc) {  // halves home, then U and sigma
    rc = s.canonicalise();
    p->held[0] = s.phys[2 * g];
    p->held[1] = s.phys[2 * g + 1];
    if (!rc && sigma) {
      const int r2 = svdj_finalize(h->dtype, p->At, h->m_pad, h->m_pad, 2 * h->B, sigma, 1, sa);
      if (r2 < 0) rc = fail(r2, "finalize: %s", svdj_hip_last_error());
    }
    if (!rc) rc = s.wait_sa();
  }
  wd.join();
  if (rc == -300 || wd.fired.load()) {
    p->comm = nullptr;  // aborted: the caller must not destroy it
    if (!rc) rc = fail(-300, "%s", wd.why);
  } else if (rc) {
    (void)hipDeviceSynchronize();  // nothing of this call may still run on its buffers
  }
  p->exchanges = s.n_exch;
  p->bytes_sent = s.n_bytes;
  if (h->timing) {
    p->comm_ms = s.comm_ms;
    p->exposed_comm_ms = exposed_time(s.waits, s.busy);
  }
  return rc;
}
