// Plan of the native distributed block one-sided Jacobi (svdj_dist.h), host
// only; svdj_dist.cpp runs it with RCCL + the HIP block kernels of
// libsvdj_hip, no Python.  Same plan as the Python engine
// (parallel/plan.py; run by parallel/pipeline.py, parallel/distributed.py):
//
// Per sweep on GPU g (slots 0 and 1 hold super-blocks of k = B/W blocks,
// each split in halves 0|1 of k/2 blocks; I = incoming slot, S = the other;
// one GPU from 64 pairs per chain step: the task pairs merged into single
// launches of twice the pairs and quad steps, as the Python engine):
//   round 0 : round robin inside each slot            (chain 0: slot 0, 1: slot 1)
//   round r : I0xS0 (0), I0xS1 (0), I1xS0 (1), send half 0 of the slot
//             replaced next, I1xS1 (1), send half 1   (last round: no sends)
// Tasks on different chains touching disjoint halves form one issue group
// (one GPU: merged into single launches); every dependency (half -> task, task ->
// send, arrival -> consumer) is a HIP event, so exchanges overlap the compute
// of the other halves (reference main.cu:582-680, 854-936 sends whole blocks
// with blocking MPI between rounds).  The stop test is an RCCL all-reduce (max
// of the float-ordered uint32 convergence value, sum of rotated pairs) per
// sweep: the value the reference computes and discards (main.cu:710).
#include "dist_plan.hpp"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <string>
#include <thread>

#include "svdj_cpu.h"
#include "svdj_debug.h"
#include "svdj_dist.h"
#include "svdj_hip.h"

namespace svdj::dist {

static thread_local char g_err[512] = {0};

int fail(int rc, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return rc;
}

Tour::Tour(int P_) : P(P_), R(2 * P_ - 1), held(R * P_ * 2), xslot(R * P_), send_to(R * P_),
                     recv_from(R * P_) {
  svdj_tournament(P, held.data(), xslot.data(), send_to.data(), recv_from.data());
}

std::vector<Item> sweep_items(const Tour& t, int g) {
  std::vector<Item> it;
  auto task = [&](int tmpl, int stream, int h0, int h1) {
    Item x;
    x.tmpl = tmpl;
    x.stream = stream;
    x.hv[0] = h0;
    x.hv[1] = h1;
    it.push_back(x);
  };
  auto send = [&](int r, int slot, int half) {
    Item x;
    x.send = true;
    x.round = r;
    x.slot = slot;
    x.half = half;
    it.push_back(x);
  };
  task(rr_template(0), 0, 0, 1);
  task(rr_template(1), 1, 2, 3);
  for (int r = 0; r < t.R; ++r) {
    const int inc = r ? t.x(r, g) : 0, stay = 1 - inc;
    auto T = [&](int ih, int sh, int stream) {
      task(cross_template(inc, ih, sh), stream, inc * 2 + ih, stay * 2 + sh);
    };
    if (r + 1 == t.R) {  // nothing to send: two fully parallel phases
      T(0, 0, 0), T(1, 1, 1), T(0, 1, 0), T(1, 0, 1);
      continue;
    }
    const int nxt = t.x(r + 1, g);
    T(0, 0, 0), T(0, 1, 0), T(1, 0, 1);
    send(r + 1, nxt, 0);
    T(1, 1, 1);
    send(r + 1, nxt, 1);
  }
  return it;
}

std::vector<Group> issue_groups(const std::vector<Item>& it) {
  std::vector<Group> out;
  const int n = (int)it.size();
  int i = 0;
  while (i < n) {
    if (!it[i].send) {
      int j = i + 1;
      while (j < n && it[j].send) ++j;
      if (j < n && j - i - 1 <= 1) {
        const Item &x = it[i], &y = it[j];
        bool ok = y.stream != x.stream;
        for (int u : x.hv)
          for (int v : y.hv) ok = ok && u != v;
        for (int s = i + 1; s < j; ++s)
          for (int v : y.hv) ok = ok && it[s].slot * 2 + it[s].half != v;
        if (ok) {
          out.push_back({i, j});
          for (int s = i + 1; s < j; ++s) out.push_back({s, -1});
          i = j + 1;
          continue;
        }
      }
    }
    out.push_back({i, -1});
    ++i;
  }
  return out;
}

PairLists pair_lists(int k, bool quad, bool merged, int cross_mode) {
  PairLists pl;
  const int hk = k / 2;
  std::vector<int32_t> rr((size_t)(k - 1) * (k / 2) * 2);
  std::vector<int32_t> rr_modes(k - 1, cross_mode);
  if (quad) {  // quad order (block.hip "quad step"): quad steps and their seconds
    svdj_quad_round_robin(k, rr.data());
    for (int s = 1; s < k - 1; ++s) rr_modes[s] = (s & 1) ? SVDJ_STEP_QUAD : SVDJ_STEP_QUAD_SECOND;
  } else {
    svdj_round_robin(k, rr.data());
  }
  rr_modes[0] = SVDJ_STEP_FULL;  // the first step of a sweep re-measures the diagonal (full Gram)
  for (int s = 0; s < 2; ++s) {
    Template& t = pl.t[rr_template(s)];
    t.pairs = rr;
    for (auto& v : t.pairs) v += s * k;
    t.steps = k - 1;
    t.npairs = k / 2;
    t.modes = rr_modes;
    t.hv[0] = 2 * s;
    t.hv[1] = 2 * s + 1;
  }
  for (int inc = 0; inc < 2; ++inc)
    for (int ih = 0; ih < 2; ++ih)
      for (int sh = 0; sh < 2; ++sh) {
        const int stay = 1 - inc;
        Template& t = pl.t[cross_template(inc, ih, sh)];
        t.pairs.assign((size_t)hk * hk * 2, 0);
        if (quad) {
          std::vector<int32_t> xs(hk), ys(hk);
          for (int a = 0; a < hk; ++a) {
            xs[a] = inc * k + ih * hk + a;
            ys[a] = stay * k + sh * hk + a;
          }
          svdj_quad_bipartite(hk, xs.data(), ys.data(), t.pairs.data());
          t.modes.assign(hk, SVDJ_STEP_QUAD);
          for (int s = 1; s < hk; s += 2) t.modes[s] = SVDJ_STEP_QUAD_SECOND;
        } else {
          for (int q = 0; q < hk; ++q)
            for (int a = 0; a < hk; ++a) {
              t.pairs[(q * hk + a) * 2] = inc * k + ih * hk + a;
              t.pairs[(q * hk + a) * 2 + 1] = stay * k + sh * hk + (a + q) % hk;
            }
          t.modes.assign(hk, cross_mode);
        }
        t.steps = hk;
        t.npairs = hk;
        t.hv[0] = inc * 2 + ih;
        t.hv[1] = stay * 2 + sh;
      }
  if (merged) {
    const int grp[3][2] = {{rr_template(0), rr_template(1)},
                           {cross_template(0, 0, 0), cross_template(0, 1, 1)},
                           {cross_template(0, 0, 1), cross_template(0, 1, 0)}};
    std::vector<int32_t>& mp = pl.merged_pairs;
    for (int m = 0; m < 3; ++m) {
      const Template &x = pl.t[grp[m][0]], &y = pl.t[grp[m][1]];
      pl.merged_off[m] = mp.size();
      pl.merged_steps[m] = x.steps;
      pl.merged_np[m] = x.npairs + y.npairs;
      pl.merged_modes[m] = x.modes;
      for (int st = 0; st < x.steps; ++st) {
        mp.insert(mp.end(), x.pairs.begin() + (size_t)st * x.npairs * 2,
                  x.pairs.begin() + (size_t)(st + 1) * x.npairs * 2);
        mp.insert(mp.end(), y.pairs.begin() + (size_t)st * y.npairs * 2,
                  y.pairs.begin() + (size_t)(st + 1) * y.npairs * 2);
      }
    }
  }
  return pl;
}

std::vector<std::pair<int, int>> placements(const int hv[2], int world) {
  // option 0: the half's home, 1: the other slot's buffer of that half, 2: the spare
  auto buffer = [](int v, int opt) { return opt == 0 ? v : opt == 1 ? 2 * (1 - v / 2) + v % 2 : 4 + v % 2; };
  std::vector<std::pair<int, int>> out;
  const int nopt = world > 1 ? 3 : 1;
  for (int ia = 0; ia < nopt; ++ia)
    for (int ib = 0; ib < nopt; ++ib)
      if (buffer(hv[0], ia) != buffer(hv[1], ib)) out.push_back({buffer(hv[0], ia), buffer(hv[1], ib)});
  return out;
}

void place_pairs(const Template& t, int k, int ba, int bb, std::vector<int32_t>& out) {
  const int hk = k / 2;
  for (int32_t v : t.pairs) {
    const int slot = v / k, rem = v % k, half = rem / hk, off = rem % hk;
    out.push_back((slot * 2 + half == t.hv[0] ? ba : bb) * hk + off);
  }
}

std::vector<std::pair<int, int>> moves_to_canonical(Layout& L) {
  std::vector<std::pair<int, int>> mv;
  for (int h = 0; h < 2; ++h) {
    int where[2] = {L.loc[0][h], L.loc[1][h]}, free_b = L.spare[h];
    for (int it = 0; it < 4; ++it) {
      int todo[2], nt = 0;
      for (int s = 0; s < 2; ++s)
        if (where[s] != 2 * s + h) todo[nt++] = s;
      if (!nt) break;
      int pick = todo[0];
      for (int q = 0; q < nt; ++q)
        if (2 * todo[q] + h == free_b) pick = todo[q];
      mv.push_back({where[pick], free_b});
      const int old = where[pick];
      where[pick] = free_b;
      free_b = old;
    }
    L.loc[0][h] = where[0];
    L.loc[1][h] = where[1];
    L.spare[h] = free_b;
  }
  return mv;
}

double exposed_time(Spans w, Spans b) {
  auto merge = [](Spans& v) {
    std::sort(v.begin(), v.end());
    Spans o;
    for (auto& x : v) {
      if (x.second <= x.first) continue;
      if (!o.empty() && x.first <= o.back().second)
        o.back().second = std::max(o.back().second, x.second);
      else
        o.push_back(x);
    }
    v.swap(o);
  };
  merge(w);
  merge(b);
  double total = 0;
  size_t j = 0;
  for (auto& x : w) {
    double t = x.first;
    while (j < b.size() && b[j].second <= t) ++j;
    size_t k = j;
    while (t < x.second) {
      if (k < b.size() && b[k].first <= t) {
        t = std::max(t, b[k].second);
        ++k;
        continue;
      }
      const double nxt = k < b.size() ? std::min(b[k].first, x.second) : x.second;
      total += nxt - t;
      t = nxt;
    }
  }
  return total;
}

namespace {

int rup(int a, int b) { return (a + b - 1) / b * b; }

// Size rule of the quad steps (hk = pairs per chain step), shared by the
// geometry's padding and svdj_dist_issue_rules (models/block.py quad_size_rule).
bool quad_size_rule(int hk, int m_pad, int world) {
  (void)m_pad;  // round 6: no row condition since the shared-GPU apply grid (profiles/r6_rule)
  return hk >= 16 || (hk >= 12 && world > 1);
}

// The id file carries a job token next to the RCCL id, so a rank accepts
// only the file of its own job attempt: SVDJ_JOB_TOKEN (svdj_dist_main --np
// sets a fresh one before forking) or torchrun's TORCHELASTIC_RUN_ID joined
// with TORCHELASTIC_RESTART_COUNT (an elastic restart, or a reused
// --rdzv-id after a crash, must not pick up the dead attempt's id).  The
// file's age is checked in every case, against the start of the reading
// process: with a token it must be younger than that minus timeout_s (a
// leftover of an older job with the same token is refused), without one
// than that minus 30 s (tokenless launchers start their ranks together and
// remove the file before their rendezvous, as bench.py does).
struct IdFile {
  char magic[8];
  char token[64];
  char id[128];  // an ncclUniqueId (svdj_dist.cpp asserts its size)
};
constexpr char kIdMagic[8] = {'S', 'V', 'D', 'J', 'I', 'D', '2', 0};

std::string job_token() {
  const char* t = getenv("SVDJ_JOB_TOKEN");
  if (t && *t) return std::string(t).substr(0, 63);
  const char* r = getenv("TORCHELASTIC_RUN_ID");
  if (r && *r && strcmp(r, "none")) {
    const char* c = getenv("TORCHELASTIC_RESTART_COUNT");
    return (std::string(r).substr(0, 48) + "#" + (c && *c ? c : "0")).substr(0, 63);
  }
  return std::string();
}

// Wall-clock start of this process (Linux /proc), or now if unavailable.
time_t process_start_time() {
  static const time_t t = [] {
    const time_t now = time(nullptr);
    long long btime = -1;
    if (FILE* f = fopen("/proc/stat", "r")) {
      char line[256];
      while (fgets(line, sizeof(line), f))
        if (!strncmp(line, "btime ", 6)) btime = atoll(line + 6);
      fclose(f);
    }
    unsigned long long start_ticks = 0;
    bool ok = false;
    if (FILE* f = fopen("/proc/self/stat", "r")) {
      char buf[1024];
      const size_t k = fread(buf, 1, sizeof(buf) - 1, f);
      fclose(f);
      buf[k] = 0;
      // field 22 (starttime) counts from the field after the ')' of comm
      if (const char* p = strrchr(buf, ')')) {
        int field = 2;
        for (const char* q = p + 1; *q && !ok; ++q)
          if (*q == ' ' && ++field == 22) ok = sscanf(q + 1, "%llu", &start_ticks) == 1;
      }
    }
    const long hz = sysconf(_SC_CLK_TCK);
    if (btime < 0 || !ok || hz <= 0) return now;
    const time_t s = (time_t)(btime + (long long)(start_ticks / (unsigned long long)hz));
    return s <= now ? s : now;
  }();
  return t;
}

}  // namespace
}  // namespace svdj::dist

using namespace svdj::dist;

extern "C" const char* svdj_dist_last_error(void) { return g_err; }

// Host part of the bootstrap (no RCCL, no GPU):
// rank 0 publishes `n` bytes at `path` (written to path.tmp, then renamed),
// every other rank waits for a fresh file of this job's token and reads them.
extern "C" int svdj_dist_id_file(int rank, const char* id_path, double timeout_s, void* blob,
                                 size_t n) {
  IdFile rec;
  if (n != sizeof(rec.id)) return fail(-2, "id blob of %zu bytes, expected %zu", n, sizeof(rec.id));
  memset(&rec, 0, sizeof(rec));
  const std::string path(id_path), token = job_token();
  if (rank == 0) {
    memcpy(rec.id, blob, n);
    memcpy(rec.magic, kIdMagic, sizeof(kIdMagic));
    memcpy(rec.token, token.data(), token.size());
    const std::string tmp = path + ".tmp";
    FILE* f = fopen(tmp.c_str(), "wb");
    if (!f) return fail(-1, "cannot write %s", tmp.c_str());
    const bool ok = fwrite(&rec, sizeof(rec), 1, f) == 1;
    fclose(f);
    if (!ok) return fail(-1, "cannot write %s", tmp.c_str());
    if (rename(tmp.c_str(), path.c_str()) != 0) return fail(-1, "cannot publish %s", path.c_str());
    return 0;
  }
  // freshness is measured from this process's start, not from this call: the
  // ranks of one launch start together, and a peer that reaches here late
  // (slow GPU init or data load) must still accept the file its rank 0
  // published after the launch
  const double window = token.empty() ? 30.0 : (timeout_s > 30 ? timeout_s : 30.0);
  const time_t not_before = process_start_time() - (time_t)window;
  const auto t0 = std::chrono::steady_clock::now();
  for (;;) {
    struct stat sb;
    const bool fresh = stat(path.c_str(), &sb) == 0 && sb.st_mtime >= not_before;
    FILE* f = fresh ? fopen(path.c_str(), "rb") : nullptr;
    if (f) {
      IdFile got;
      const size_t k = fread(&got, sizeof(got), 1, f);
      fclose(f);
      if (k == 1 && !memcmp(got.magic, kIdMagic, sizeof(kIdMagic)) &&
          !strncmp(got.token, token.c_str(), sizeof(got.token))) {
        memcpy(blob, got.id, n);
        return 0;
      }
    }
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (el > timeout_s)
      return fail(-2, "rank %d: no unique id of this job (token '%s') at %s after %.0f s", rank,
                  token.c_str(), path.c_str(), el);
    std::this_thread::sleep_for(std::chrono::milliseconds(20));
  }
}

extern "C" int svdj_dist_geometry(int world, int m, int n, int W, int dtype, int* B, int* ncols,
                                  int* m_pad, int* n_v) {
  if (world < 1 || m < n || n < 1 || (W != 32 && W != 64) || dtype < 0 || dtype > 2)
    return fail(-2, "bad geometry args");
  const int q = 4 * world * W;  // B/W even: super-blocks split in halves
  int nc = rup(n > q ? n : q, q);
  const int mp = rup(m, SVDJ_ROW_ALIGN);
  // quad steps need k = B/W % 4 == 0: a column count that lands on k % 4 == 2
  // where the quad rule would hold takes one more q of zero columns (<= 6 %
  // more columns at the sizes the rule admits; quad vs single steps is 20-25 %
  // per solve).  Not for fp64 (no quad steps).  distributed.py geometry.
  if (dtype != 1 && W == 64 && svdj_debug_knob("quad_pad", 1) != 0) {
    const int k = nc / (2 * world * W);
    if (k % 4 == 2 && quad_size_rule((k + 2) / 2, mp, world)) nc += q;
  }
  *ncols = nc;
  *B = nc / (2 * world);
  *m_pad = mp;
  *n_v = rup(nc, SVDJ_ROW_ALIGN);
  return 0;
}

extern "C" int svdj_dist_choose_block(int dtype, int world, int m, int n) {
  // models/block.py choose_block (measurements there)
  const int per_gpu = n / (world > 0 ? world : 1);
  if (dtype == 1) return (m >= 6144 && per_gpu >= 2048) ? 64 : 32;
  return per_gpu >= 1024 ? 64 : 32;
}

extern "C" int svdj_dist_initial_held(int world, int rank, int32_t held[2]) {
  Tour t(world);
  held[0] = t.h(0, rank, 0);
  held[1] = t.h(0, rank, 1);
  return 0;
}

extern "C" int svdj_dist_storage_cols(int world, int B) { return (world > 1 ? 3 : 2) * B; }

extern "C" int svdj_dist_plan(int world, int rank, int32_t* out, int cap) {
  if (world < 1 || rank < 0 || rank >= world) return fail(-2, "bad plan args");
  const std::vector<Item> items = sweep_items(Tour(world), rank);
  const std::vector<Group> groups = issue_groups(items);
  if ((int)groups.size() > cap) return fail(-2, "plan has %zu groups, cap %d", groups.size(), cap);
  for (size_t i = 0; i < groups.size(); ++i) {
    int32_t* o = out + 7 * i;
    const Item& a = items[groups[i].a];
    for (int j = 0; j < 7; ++j) o[j] = -1;
    if (a.send) {
      o[0] = 2, o[1] = a.round, o[2] = a.slot, o[3] = a.half;
      continue;
    }
    o[0] = groups[i].b < 0 ? 0 : 1;
    o[1] = a.stream, o[2] = a.hv[0], o[3] = a.hv[1];
    if (groups[i].b >= 0) {
      const Item& b = items[groups[i].b];
      o[4] = b.stream, o[5] = b.hv[0], o[6] = b.hv[1];
    }
  }
  return (int)groups.size();
}

extern "C" int svdj_dist_issue_rules(int world, int dtype, int W, int mma, int k, int m_pad,
                                     int quad_mode, int* quad, int* merged) {
  const bool quad_ok = dtype == 0 && W == 64 && svdj_mma_parts(mma) && k % 4 == 0;
  if (quad_mode < 0 || quad_mode > 2) return fail(-2, "quad %d (0 auto, 1 on, 2 off)", quad_mode);
  if (quad_mode == 1 && !quad_ok)
    return fail(-2, "quad steps need fp32, W = 64, a split-bf16 apply and k %% 4 == 0");
  // models/block.py choose_quad, choose_merged
  const int hk = k / 2;
  *quad = quad_ok && (quad_mode == 1 || (quad_mode == 0 && quad_size_rule(hk, m_pad, world)));
  const int force = svdj_debug_knob("merge", -1);  // A/B only (svdj_debug.h), world 1 only
  *merged = world == 1 && (force >= 0 ? force == 1 : *quad ? (hk >= 16 && hk < 32) : hk >= 64);
  return 0;
}

extern "C" int svdj_dist_merged_lists(int k, int quad, int cross_mode, int32_t* pairs, int pcap,
                                      int32_t* modes, int mcap, int32_t* meta) {
  if (k < 4 || k % 2 || (quad && k % 4)) return fail(-2, "bad merged-list args");
  const PairLists pl = pair_lists(k, quad != 0, true, cross_mode);
  size_t nm = 0;
  for (int m = 0; m < 3; ++m) nm += pl.merged_modes[m].size();
  if (pl.merged_pairs.size() > (size_t)pcap || nm > (size_t)mcap)
    return fail(-3, "merged lists: buffer too small");
  std::copy(pl.merged_pairs.begin(), pl.merged_pairs.end(), pairs);
  for (int m = 0, at = 0; m < 3; ++m) {
    meta[m * 3] = (int32_t)pl.merged_off[m];
    meta[m * 3 + 1] = pl.merged_steps[m];
    meta[m * 3 + 2] = pl.merged_np[m];
    for (int32_t v : pl.merged_modes[m]) modes[at++] = v;
  }
  return (int)pl.merged_pairs.size();
}
