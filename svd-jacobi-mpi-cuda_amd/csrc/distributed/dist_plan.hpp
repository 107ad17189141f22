// Host side of the native distributed engine (dist_plan.cpp): the sweep plan,
// the pair lists of its templates, the placement of the halves and the timing
// arithmetic.  No HIP, no RCCL: svdj_dist.cpp enqueues what is planned here,
// and tools/micro/dist_plan_check.cpp runs it alone under ASan + UBSan.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

namespace svdj::dist {

// Records the calling thread's message (svdj_dist_last_error) and returns rc.
int fail(int rc, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

struct Tour {  // svdj_tournament of P GPUs: 2P - 1 rounds
  int P, R;
  std::vector<int32_t> held, xslot, send_to, recv_from;
  explicit Tour(int P);
  int h(int r, int g, int s) const { return held[(r * P + g) * 2 + s]; }
  int x(int r, int g) const { return xslot[r * P + g]; }
  int to(int r, int g) const { return send_to[r * P + g]; }
  int from(int r, int g) const { return recv_from[r * P + g]; }
};

// ---- sweep plan of one GPU (parallel/plan.py sweep_plan / issue_groups)
// Halves are keyed slot*2 + half.  A task runs one template on a stream
// (chain); a Send moves one half of one slot.
enum { kTemplates = 10 };  // rr of slot 0, 1; cross[inc][ih][sh]
inline int rr_template(int slot) { return slot; }
inline int cross_template(int inc, int ih, int sh) { return 2 + inc * 4 + ih * 2 + sh; }

struct Item {
  bool send = false;
  int tmpl = -1, stream = 0, hv[2] = {0, 0};  // task: template, chain, the two halves it touches
  int round = 0, slot = 0, half = 0;          // send
};
std::vector<Item> sweep_items(const Tour& t, int g);

// Issue order: a task is paired with the next task (at most one Send in
// between) when they run on different chains, touch disjoint halves and the
// Send concerns neither half of the second; the Send is issued after the pair.
struct Group {
  int a = -1, b = -1;  // item indices (b = -1: single task; a is a Send if items[a].send)
};
std::vector<Group> issue_groups(const std::vector<Item>& it);

// ---- pair lists.  A chain template: pairs in canonical local block ids
// (slot*k + half*hk + j), one mode per step, and the two halves it touches.
struct Template {
  std::vector<int32_t> pairs, modes;
  int steps = 0, npairs = 0;
  int hv[2] = {0, 0};  // halves touched (slot*2 + half)
};
// One GPU (canonical buffers: a local block id is its buffer block): the
// parallel task pairs of the sweep -- rr0 + rr1, then the last round's
// [T00 || T11] and [T01 || T10] -- concatenated step by step, the order of
// pipeline.py run_merged.  List i starts at pairs[off[i]].
struct PairLists {
  Template t[kTemplates];
  std::vector<int32_t> merged_pairs, merged_modes[3];
  size_t merged_off[3] = {0, 0, 0};
  int merged_steps[3] = {0, 0, 0}, merged_np[3] = {0, 0, 0};
};
PairLists pair_lists(int k, bool quad, bool merged, int cross_mode);

// Every placement of a template's two halves: half h lives in one of buffers
// {h, 2+h, 4+h} (only the canonical ones on one GPU).  {buffer of hv[0],
// buffer of hv[1]}, never equal.
std::vector<std::pair<int, int>> placements(const int hv[2], int world);
// Physical block ids (buffer*hk + offset) of a template's canonical ids with
// its halves in buffers ba, bb; appended to out.
void place_pairs(const Template& t, int k, int ba, int bb, std::vector<int32_t>& out);

// ---- where the resident halves live (parallel/plan.py HalfLayout).
// Half buffers of hB columns: loc[slot][half] holds (slot, half); spare[h] is
// the free buffer the next exchange of a half h receives into.  Buffers
// {h, 2+h, 4+h} always hold (slot 0, h), (slot 1, h), spare.
struct Layout {
  int loc[2][2] = {{0, 1}, {2, 3}};
  int spare[2] = {4, 5};
};
// Moves (src buffer, dst buffer) that bring every half home to buffer
// 2 slot + half, parking one half in the spare when two sit in each other's
// home (same rule as HalfLayout.moves_to_canonical).
std::vector<std::pair<int, int>> moves_to_canonical(Layout& L);

// Interval measure of union(waits) minus union(busy) (plan.exposed_time).
using Spans = std::vector<std::pair<double, double>>;
double exposed_time(Spans waits, Spans busy);

}  // namespace svdj::dist
