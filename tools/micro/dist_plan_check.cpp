// Host-only check of the native engine's plan unit (csrc/distributed/dist_plan.cpp)
// under AddressSanitizer + UBSan: the sweep plan, the pair lists, the placement
// remap, moves_to_canonical, exposed_time, the id file, geometry and issue
// rules.  No HIP, no RCCL, no Python; tests/test_dist_plan_cpu.py builds and
// runs it.
//
//   g++ -fsanitize=address,undefined -fno-omit-frame-pointer -O1 -g -std=c++17 -Wall
//     -I svd-jacobi-mpi-cuda_amd/csrc/include -I svd-jacobi-mpi-cuda_amd/csrc/distributed
//     tools/micro/dist_plan_check.cpp svd-jacobi-mpi-cuda_amd/csrc/distributed/dist_plan.cpp
//     svd-jacobi-mpi-cuda_amd/csrc/cpu/schedule.cpp -o dist_plan_check
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <map>
#include <string>

#include "dist_plan.hpp"
#include "svdj_dist.h"
#include "svdj_hip.h"

using namespace svdj::dist;

static int g_cases = 0, g_bad = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      ++g_bad;                                 \
      printf("FAILED %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                     \
      printf("\n");                            \
    }                                          \
  } while (0)

static void check_plan() {
  for (int P = 1; P <= 8; ++P)
    for (int g = 0; g < P; ++g, ++g_cases) {
      std::vector<int32_t> rows(7 * (64 * P + 16), -7);
      const int n = svdj_dist_plan(P, g, rows.data(), 64 * P + 16);
      CHECK(n > 0, "plan P=%d g=%d: %d", P, g, n);
      if (n <= 0) continue;
      std::vector<int32_t> exact(7 * n);  // ASan: a row past cap is a heap overflow
      CHECK(svdj_dist_plan(P, g, exact.data(), n) == n, "plan P=%d g=%d: exact cap refused", P, g);
      CHECK(svdj_dist_plan(P, g, exact.data(), n - 1) < 0, "plan P=%d g=%d: cap - 1 accepted", P, g);
      CHECK(!memcmp(exact.data(), rows.data(), exact.size() * 4), "plan P=%d g=%d differs", P, g);
      std::map<int, std::vector<int>> sent;  // round -> halves in issue order
      for (int i = 0; i < n; ++i) {
        const int32_t* o = &exact[7 * i];
        if (o[0] == 2) sent[o[1]].push_back(o[3]);
        if (o[0] != 1) continue;
        CHECK(o[1] != o[4], "P=%d g=%d group %d: both tasks on chain %d", P, g, i, o[1]);
        CHECK(o[2] != o[5] && o[2] != o[6] && o[3] != o[5] && o[3] != o[6],
              "P=%d g=%d group %d: tasks share a half", P, g, i);
      }
      CHECK((int)sent.size() == 2 * P - 2, "P=%d g=%d: sends in %zu rounds", P, g, sent.size());
      for (auto& s : sent)
        CHECK(s.second == std::vector<int>({0, 1}), "P=%d g=%d round %d: halves not sent 0, 1", P, g,
              s.first);
    }
}

static void check_pair_lists() {
  for (int k : {4, 6, 8, 12, 16, 32, 64})
    for (int quad = 0; quad < (k % 4 == 0 ? 2 : 1); ++quad, ++g_cases) {
      const int hk = k / 2, cm = SVDJ_STEP_CROSS_BIP;
      const PairLists pl = pair_lists(k, quad != 0, true, cm);
      for (const Template& t : pl.t) {
        CHECK((int)t.modes.size() == t.steps, "k=%d quad=%d: %zu modes, %d steps", k, quad,
              t.modes.size(), t.steps);
        CHECK(t.pairs.size() == (size_t)t.steps * t.npairs * 2, "k=%d quad=%d: pair count", k, quad);
      }
      for (int inc = 0; inc < 2; ++inc) {  // one round's templates meet every pair exactly once
        std::vector<int> met(4 * k * k, 0);
        std::vector<int> ts = {rr_template(0), rr_template(1)};
        for (int q = 0; q < 4; ++q) ts.push_back(cross_template(inc, q / 2, q % 2));
        bool in_range = true;
        for (int t : ts)
          for (size_t i = 0; i < pl.t[t].pairs.size() && in_range; i += 2) {
            const int a = pl.t[t].pairs[i], b = pl.t[t].pairs[i + 1];
            in_range = a >= 0 && b >= 0 && a < 2 * k && b < 2 * k && a != b;
            if (in_range) ++met[std::min(a, b) * 2 * k + std::max(a, b)];
          }
        CHECK(in_range, "k=%d quad=%d inc=%d: block id out of range", k, quad, inc);
        int wrong = 0;
        for (int a = 0; a < 2 * k; ++a)
          for (int b = a + 1; b < 2 * k; ++b) wrong += met[a * 2 * k + b] != 1;
        CHECK(!wrong, "k=%d quad=%d inc=%d: %d pairs not met exactly once", k, quad, inc, wrong);
      }
      // merged lists: the step-wise concatenation of their two templates
      const int grp[3][2] = {{rr_template(0), rr_template(1)},
                             {cross_template(0, 0, 0), cross_template(0, 1, 1)},
                             {cross_template(0, 0, 1), cross_template(0, 1, 0)}};
      size_t at = 0;
      for (int m = 0; m < 3; ++m) {
        const Template &x = pl.t[grp[m][0]], &y = pl.t[grp[m][1]];
        CHECK(pl.merged_off[m] == at && pl.merged_steps[m] == x.steps && x.steps == y.steps &&
                  pl.merged_np[m] == x.npairs + y.npairs && pl.merged_modes[m] == x.modes,
              "k=%d quad=%d merged list %d: meta", k, quad, m);
        std::vector<int32_t> want;
        for (int st = 0; st < x.steps; ++st)
          for (const Template* t : {&x, &y})
            for (int i = 0; i < t->npairs * 2; ++i) want.push_back(t->pairs[(size_t)st * t->npairs * 2 + i]);
        CHECK(at + want.size() <= pl.merged_pairs.size() &&
                  std::equal(want.begin(), want.end(), pl.merged_pairs.begin() + at),
              "k=%d quad=%d merged list %d: pairs", k, quad, m);
        at += want.size();
      }
      CHECK(at == pl.merged_pairs.size(), "k=%d quad=%d: merged pairs end", k, quad);
      CHECK(pair_lists(k, quad != 0, false, cm).merged_pairs.empty(), "unmerged lists not empty");
      // the exported view of the same lists, into buffers of exactly their sizes
      std::vector<int32_t> pairs(at), modes(2 * hk + k - 1), meta(9);
      CHECK(svdj_dist_merged_lists(k, quad, cm, pairs.data(), (int)at, modes.data(), (int)modes.size(),
                                   meta.data()) == (int)at && pairs == pl.merged_pairs,
            "k=%d quad=%d: svdj_dist_merged_lists", k, quad);
      CHECK(svdj_dist_merged_lists(k, quad, cm, pairs.data(), (int)at - 1, modes.data(),
                                   (int)modes.size(), meta.data()) < 0, "short pair buffer accepted");
    }
}

static void check_placements() {
  const int k = 8, hk = 4;
  const PairLists pl = pair_lists(k, false, false, SVDJ_STEP_CROSS);
  for (int world : {1, 2})
    for (const Template& t : pl.t) {
      const auto pls = placements(t.hv, world);
      const size_t want = world == 1 ? 1 : (t.hv[0] % 2 == t.hv[1] % 2 ? 6 : 9);
      CHECK(pls.size() == want, "world %d halves (%d, %d): %zu placements", world, t.hv[0], t.hv[1],
            pls.size());
      if (world == 1) CHECK(pls[0] == std::make_pair(t.hv[0], t.hv[1]), "world 1: not canonical");
      for (auto [ba, bb] : pls) {
        ++g_cases;
        CHECK(ba != bb && ba % 2 == t.hv[0] % 2 && bb % 2 == t.hv[1] % 2 && ba >= 0 && ba < 6 &&
                  bb >= 0 && bb < 6, "halves (%d, %d) in buffers (%d, %d)", t.hv[0], t.hv[1], ba, bb);
        std::vector<int32_t> phys;
        place_pairs(t, k, ba, bb, phys);
        CHECK(phys.size() == t.pairs.size(), "placement changes the pair count");
        for (size_t i = 0; i < phys.size() && i < t.pairs.size(); ++i) {
          const int v = t.pairs[i], half = v / k * 2 + v % k / hk;
          CHECK(half == t.hv[0] || half == t.hv[1], "id %d outside the template's halves", v);
          CHECK(phys[i] / hk == (half == t.hv[0] ? ba : bb) && phys[i] % hk == v % hk,
                "id %d placed at %d (buffers %d, %d)", v, phys[i], ba, bb);
        }
      }
    }
}

static void check_moves() {
  const int perm[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};
  for (int p0 = 0; p0 < 6; ++p0)
    for (int p1 = 0; p1 < 6; ++p1, ++g_cases) {
      Layout L;
      int label[6] = {-1, -1, -1, -1, -1, -1};  // buffer -> half held (slot*2 + half), -1 free
      for (int h = 0; h < 2; ++h) {
        const int* pm = perm[h ? p1 : p0];  // buffers {h, 2+h, 4+h} over (slot 0, slot 1, spare)
        L.loc[0][h] = 2 * pm[0] + h;
        L.loc[1][h] = 2 * pm[1] + h;
        L.spare[h] = 2 * pm[2] + h;
        label[L.loc[0][h]] = h;
        label[L.loc[1][h]] = 2 + h;
      }
      const auto moves = moves_to_canonical(L);
      CHECK(moves.size() <= 6, "layout %d/%d: %zu moves", p0, p1, moves.size());
      for (auto [src, dst] : moves) {
        CHECK(src >= 0 && src < 6 && dst >= 0 && dst < 6 && src != dst, "move %d -> %d", src, dst);
        CHECK(label[dst] == -1, "layout %d/%d: copy %d -> %d overwrites live half %d", p0, p1, src, dst,
              label[dst]);
        label[dst] = label[src];
        label[src] = -1;
      }
      for (int b = 0; b < 6; ++b)
        CHECK(label[b] == (b < 4 ? b : -1), "layout %d/%d: buffer %d ends with %d", p0, p1, b, label[b]);
      const Layout home;
      CHECK(!memcmp(L.loc, home.loc, sizeof(L.loc)) && !memcmp(L.spare, home.spare, sizeof(L.spare)),
            "layout %d/%d: layout not canonical after the moves", p0, p1);
    }
}

static void check_exposed_time() {
  struct Case {
    const char* name;
    Spans waits, busy;
    double want;  // worked out by hand; every value is exact in binary
  };
  const Case cases[] = {
      {"nothing", {}, {}, 0},
      {"no wait", {}, {{0, 1}}, 0},
      {"no task", {{0, 2}}, {}, 2},
      {"empty wait", {{3, 3}, {5, 4}}, {}, 0},
      {"fully covered", {{1, 2}}, {{0, 3}}, 0},                // [1,2] inside [0,3]
      {"partly covered", {{1, 4}}, {{0, 2}}, 2},               // [2,4] is exposed
      {"covered in the middle", {{0, 4}}, {{1, 2}}, 3},        // [0,1] + [2,4]
      {"nested busy", {{0, 10}}, {{2, 3}, {2.25, 2.75}, {5, 6}}, 8},  // 10 - [2,3] - [5,6]
      {"nested waits", {{0, 4}, {1, 2}}, {{3, 8}}, 3},         // union [0,4] minus [3,8]
      {"touching", {{0, 1}, {1, 2}}, {{0.5, 1}, {1, 1.5}}, 1},  // [0,2] minus [0.5,1.5]
      {"busy touches the wait's ends", {{1, 2}}, {{0, 1}, {2, 3}}, 1},
      {"two waits, one busy across", {{0, 2}, {4, 6}}, {{1, 5}}, 2},  // [0,1] + [5,6]
      {"unsorted", {{4, 6}, {0, 2}}, {{5, 7}, {1, 3}}, 2},     // [0,1] + [4,5]
  };
  for (const Case& c : cases) {
    ++g_cases;
    const double got = exposed_time(c.waits, c.busy);
    CHECK(got == c.want, "exposed_time %s: %g, expected %g", c.name, got, c.want);
  }
}

static void check_id_file() {
  char dir[] = "/tmp/dist_plan_check.XXXXXX";
  if (!mkdtemp(dir)) {
    CHECK(false, "mkdtemp failed");
    return;
  }
  const std::string path = std::string(dir) + "/id", missing = std::string(dir) + "/none";
  unsigned char id[128], back[128] = {0}, small[64] = {0};
  for (int i = 0; i < 128; ++i) id[i] = (unsigned char)(i * 7 + 1);
  setenv("SVDJ_JOB_TOKEN", "job-a", 1);
  CHECK(svdj_dist_id_file(0, path.c_str(), 5.0, id, sizeof(id)) == 0, "rank 0: %s", svdj_dist_last_error());
  CHECK(svdj_dist_id_file(1, path.c_str(), 5.0, back, sizeof(back)) == 0 && !memcmp(id, back, 128),
        "rank 1 did not read the id back: %s", svdj_dist_last_error());
  struct stat sb;
  CHECK(stat(path.c_str(), &sb) == 0 && sb.st_size == 8 + 64 + 128, "id file size");
  unsigned char raw[200] = {0};
  if (FILE* f = fopen(path.c_str(), "rb")) {
    CHECK(fread(raw, 1, 200, f) == 200, "id file short");
    fclose(f);
  }
  CHECK(!memcmp(raw, "SVDJID2", 8) && !strcmp((char*)raw + 8, "job-a") && !memcmp(raw + 72, id, 128),
        "id file is not magic | token | id");
  CHECK(svdj_dist_id_file(0, path.c_str(), 0.2, small, sizeof(small)) == -2, "64-byte blob written");
  CHECK(svdj_dist_id_file(1, path.c_str(), 0.2, small, sizeof(small)) == -2, "64-byte blob read");
  CHECK(svdj_dist_id_file(1, missing.c_str(), 0.2, back, sizeof(back)) == -2, "missing file accepted");
  setenv("SVDJ_JOB_TOKEN", "job-b", 1);
  CHECK(svdj_dist_id_file(1, path.c_str(), 0.2, back, sizeof(back)) == -2, "another job's file accepted");
  unsetenv("SVDJ_JOB_TOKEN");
  unlink(path.c_str());
  unlink((path + ".tmp").c_str());
  rmdir(dir);
  g_cases += 5;
}

static void check_geometry_and_rules() {
  for (int world : {1, 2, 4, 8})
    for (int W : {32, 64})
      for (int dtype = 0; dtype < 3; ++dtype) {
        const int q = 4 * world * W;
        for (int mult : {1, 2, 3, 9, 17, 18})
          for (int d = -1; d <= 1; ++d, ++g_cases) {
            const int n = mult * q + d;
            int B = 0, ncols = 0, m_pad = 0, n_v = 0;
            CHECK(svdj_dist_geometry(world, n, n, W, dtype, &B, &ncols, &m_pad, &n_v) == 0,
                  "geometry world %d W %d n %d", world, W, n);
            CHECK(ncols % q == 0 && ncols >= n && ncols < n + 2 * q && 2 * world * B == ncols,
                  "world %d W %d dtype %d n %d: ncols %d B %d", world, W, dtype, n, ncols, B);
            CHECK(m_pad >= n && m_pad % SVDJ_ROW_ALIGN == 0 && n_v >= ncols && n_v % SVDJ_ROW_ALIGN == 0,
                  "world %d W %d n %d: m_pad %d n_v %d", world, W, n, m_pad, n_v);
            if (dtype == 2) continue;  // the rules know fp32 and fp64
            const int k = B / W;
            for (int mma = 0; mma < 3; ++mma)
              for (int mode = 0; mode < 3; ++mode) {
                int quad = -1, merged = -1;
                const int rc = svdj_dist_issue_rules(world, dtype, W, mma, k, m_pad, mode, &quad, &merged);
                if (rc < 0) {
                  CHECK(mode == 1, "rules refused mode %d (world %d W %d k %d)", mode, world, W, k);
                  continue;
                }
                CHECK((quad == 0 || quad == 1) && (merged == 0 || merged == 1), "rules: not 0 / 1");
                CHECK(!quad || (k % 4 == 0 && mode != 2), "quad steps at k = %d, mode %d", k, mode);
                CHECK(!merged || world == 1, "merged issue on %d GPUs", world);
              }
          }
      }
  int B, ncols, m_pad, n_v;
  CHECK(svdj_dist_geometry(1, 64, 128, 64, 0, &B, &ncols, &m_pad, &n_v) < 0, "m < n accepted");
  CHECK(svdj_dist_geometry(1, 128, 128, 48, 0, &B, &ncols, &m_pad, &n_v) < 0, "W = 48 accepted");
}

int main() {
  check_plan();
  check_pair_lists();
  check_placements();
  check_moves();
  check_exposed_time();
  check_id_file();
  check_geometry_and_rules();
  printf("%d cases checked, %d checks failed\n", g_cases, g_bad);
  return g_bad != 0;
}
