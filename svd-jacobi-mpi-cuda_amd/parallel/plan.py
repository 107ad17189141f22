"""Half-block pipelined sweep: the plan, host only (no torch).

The tournament (schedule.tournament) replaces ONE resident super-block per
GPU between rounds.  Every super-block is handled as two halves and a round's
cross work is four half-pair tasks (I = incoming slot, S = staying slot):

    stream 0:  T00 = I0 x S0   ->  T01 = I0 x S1
    stream 1:  T10 = I1 x S0   ->  T11 = I1 x S1

Half 0 of the next outgoing slot is last touched by T01/T10, half 1 by T11,
so the send/recv of half 0 is issued right after T10 and runs under T11;
half 1 is issued after T11 and runs under the next round's T00' and T01'
(which only need the already-arrived half 0).  Round 0 of every sweep also
runs the within-super-block round robins (RR(slot 0) || RR(slot 1)); the last
round of a sweep (no exchange after it, the whole sweep on one GPU) runs the
fully parallel order [T00 || T11], [T01 || T10].  Every block pair of the
matrix still meets exactly once per sweep (tests/test_pipeline_cpu.py).
parallel/pipeline.py executes a plan; csrc/distributed/dist_plan.cpp is the
native twin of this module.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from ..ops.codes import STEP_CROSS, STEP_FULL
from .schedule import (quad_bipartite, quad_bipartite_modes, quad_round_robin,
                       quad_round_robin_modes, round_robin)


@dataclass
class Task:
    """One chain of block steps on local block indices."""
    name: str
    pairs: np.ndarray        # (steps, pairs_per_step, 2)
    modes: list
    stream: int
    halves: tuple            # ((slot, part), ...) touched (parts are halves for 2 chains)


@dataclass
class Send:
    """Exchange of part ``half`` of slot ``slot`` before round ``round``."""
    round: int
    slot: int
    half: int


@dataclass
class SweepPlan:
    P: int
    k: int
    items: list = field(default_factory=list)   # Task | Send, in issue order
    parts: int = 2           # a super-block moves in this many parts (= chains)


def _blocks(slot: int, half: int, k: int, parts: int = 2) -> list:
    h = k // parts
    return list(range(slot * k + half * h, slot * k + (half + 1) * h))


def _bipartite(xs: list, ys: list) -> np.ndarray:
    h = len(xs)
    out = np.zeros((h, h, 2), dtype=np.int32)
    for t in range(h):
        for a in range(h):
            out[t, a] = (xs[a], ys[(a + t) % h])
    return out


def sweep_plan(P: int, k: int, xslot: np.ndarray, chains: int = 2, quad: bool = False
               ) -> SweepPlan:
    """Items of one sweep.  ``xslot[r]`` is the slot replaced before round r
    (r >= 1), as produced by schedule.tournament.  (Four chains in quarters
    were measured slower than two at every P in round 2 -- 8-GPU plan 64 ->
    84-88 ms per sweep -- and removed.)  ``quad``: the same block pairs in
    quad order (schedule.quad_round_robin / quad_bipartite, mode 4/5 steps
    fused two at a time, csrc/hip/block.hip "quad step"); needs k % 4 == 0."""
    if chains != 2:
        raise ValueError(f"pipelined sweep: 2 chains, got {chains}")
    if k < 2 or k % 2:
        raise ValueError(f"pipelined sweep needs an even block count per super-block, got {k}")
    if quad and k % 4:
        raise ValueError(f"quad steps need a multiple of 4 blocks per super-block, got {k}")
    plan = SweepPlan(P, k)
    if quad:
        rr, rr_modes = quad_round_robin(k), quad_round_robin_modes(k)
    else:
        rr, rr_modes = round_robin(k), [STEP_FULL] + [STEP_CROSS] * (k - 2)
    plan.items.append(Task("rr0", rr.copy(), rr_modes, 0, ((0, 0), (0, 1))))
    plan.items.append(Task("rr1", rr + k, rr_modes, 1, ((1, 0), (1, 1))))
    R = 2 * P - 1
    for r in range(R):
        inc = int(xslot[r]) if r > 0 else 0
        stay = 1 - inc
        h = k // 2

        def task(name, ih, sh, stream):
            xs, ys = _blocks(inc, ih, k), _blocks(stay, sh, k)
            if quad:
                return Task(f"r{r}.{name}", quad_bipartite(xs, ys), quad_bipartite_modes(h), stream,
                            ((inc, ih), (stay, sh)))
            return Task(f"r{r}.{name}", _bipartite(xs, ys), [STEP_CROSS] * h, stream,
                        ((inc, ih), (stay, sh)))

        nxt = int(xslot[r + 1]) if r + 1 < R else None
        if nxt is None:
            # nothing to send after this round: the two fully parallel phases
            # [T00 || T11], [T01 || T10]
            plan.items += [task("T00", 0, 0, 0), task("T11", 1, 1, 1), task("T01", 0, 1, 0),
                           task("T10", 1, 0, 1)]
            continue
        plan.items += [task("T00", 0, 0, 0), task("T01", 0, 1, 0), task("T10", 1, 0, 1),
                       Send(r + 1, nxt, 0), task("T11", 1, 1, 1), Send(r + 1, nxt, 1)]
    return plan


def issue_groups(items: list, joint: bool, max_group: int = 2) -> list:
    """The plan's items regrouped for issue: a Task, a Send, or a tuple of up
    to ``max_group`` independent tasks issued jointly (merged into single
    launches on one GPU, :meth:`PipelineExecutor.run_merged`).

    Greedy: a task is grouped with the following tasks (Sends in between are
    skipped) while each runs on a new stream, touches parts disjoint from the
    group's, and no skipped Send concerns its parts; the skipped Sends are
    issued after the group (they only wait on events of earlier users of
    their part, so the delay is host-side only).  For two chains this pairs
    rr0+rr1, T01+T10, the last round's T00+T11 / T01+T10, and T11 of a round
    with T00 of the next across the half-1 Send."""
    out = []
    i, n = 0, len(items)
    while i < n:
        it = items[i]
        if not (joint and isinstance(it, Task)):
            out.append(it)
            i += 1
            continue
        group, streams, parts = [it], {it.stream}, set(it.halves)
        skipped, last, j = [], i, i + 1
        while j < n and len(group) < max_group:
            x = items[j]
            if isinstance(x, Send):
                skipped.append((j, x))
                j += 1
                continue
            if (x.stream in streams or set(x.halves) & parts
                    or any((sd.slot, sd.half) in x.halves for _, sd in skipped)):
                break
            group.append(x)
            streams.add(x.stream)
            parts |= set(x.halves)
            last = j
            j += 1
        out.append(tuple(group) if len(group) > 1 else it)
        out.extend(sd for idx, sd in skipped if idx < last)
        i = last + 1
    return out


def check_plan_coverage(plans: list, tour) -> None:
    """Simulate one sweep on every GPU (``plans[g]`` is GPU g's plan; all have
    the same item structure) on global block ids, from the tournament's
    starting placement; assert that every pair of global blocks meets
    exactly once.  Raises AssertionError."""
    P = len(plans)
    k = plans[0].k
    parts = plans[0].parts
    h = k // parts
    # place[g][slot][part] = (super-block, part) currently resident
    place = [[[(int(tour.held[0, g, s]), hh) for hh in range(parts)] for s in range(2)]
             for g in range(P)]
    met = {}
    n_items = len(plans[0].items)
    assert all(len(p.items) == n_items for p in plans)
    for i in range(n_items):
        its = [p.items[i] for p in plans]
        if isinstance(its[0], Send):
            assert all(isinstance(x, Send) and x.half == its[0].half and x.round == its[0].round
                       for x in its)
            r, hh = its[0].round, its[0].half
            new = [None] * P
            for g in range(P):
                src = int(tour.recv_from[r, g])
                assert int(tour.send_to[r, src]) == g
                new[g] = place[src][its[src].slot][hh]
            for g in range(P):
                place[g][its[g].slot][hh] = new[g]
            continue
        for g in range(P):
            it = its[g]
            for t in range(it.pairs.shape[0]):
                for a, b in it.pairs[t]:
                    ga = _global_block(place[g], int(a), k, h)
                    gb = _global_block(place[g], int(b), k, h)
                    assert ga != gb
                    key = (min(ga, gb), max(ga, gb))
                    met[key] = met.get(key, 0) + 1
    nb = 2 * P * k
    assert len(met) == nb * (nb - 1) // 2, (len(met), nb * (nb - 1) // 2)
    assert all(v == 1 for v in met.values())


def _global_block(place_g, b: int, k: int, h: int) -> int:
    slot, rem = divmod(b, k)
    half, off = divmod(rem, h)
    sb, hh = place_g[slot][half]
    return sb * k + hh * h + off


def _union(iv: list) -> list:
    """Sorted, merged union of (start, end) intervals."""
    out = []
    for a, b in sorted(x for x in iv if x[1] > x[0]):
        if out and a <= out[-1][1]:
            out[-1][1] = max(out[-1][1], b)
        else:
            out.append([a, b])
    return out


def exposed_time(waits: list, busy: list) -> float:
    """Measure of the time covered by some wait interval (a compute stream
    idle until an exchange arrives) and by NO busy interval (a task running
    on any compute stream of the rank): each moment counts once, however many
    consumers wait on the arrival and on however many streams."""
    w, b = _union(waits), _union(busy)
    total, j = 0.0, 0
    for ws, we in w:
        t = ws
        while j < len(b) and b[j][1] <= t:
            j += 1
        k = j
        while t < we:
            if k < len(b) and b[k][0] <= t:
                t = max(t, b[k][1])
                k += 1
                continue
            nxt = b[k][0] if k < len(b) else we
            total += min(nxt, we) - t
            t = min(nxt, we)
    return total


class HalfLayout:
    """Where each resident half super-block lives: the rank's storage is a
    row of half buffers (hB columns each): loc[slot][half] is the buffer of
    (slot, half), spare[half] the free buffer that the next exchange of a
    half ``half`` receives into.  An exchange sends from loc[x][h], receives
    into spare[h] and swaps the two -- the received columns are used where
    they landed, no copy (round 2 received into a staging buffer and copied
    it into place: 654 copy dispatches per 8-GPU rank-plan profile).
    Buffers {h, 2 + h, 4 + h} always hold (slot 0, h), (slot 1, h), spare."""

    def __init__(self, spares: bool):
        self.loc = [[0, 1], [2, 3]]
        self.spare = [4, 5] if spares else None

    @property
    def nbuf(self) -> int:
        return 6 if self.spare is not None else 4

    def canonical(self) -> bool:
        return self.loc == [[0, 1], [2, 3]]

    def table(self, k: int) -> np.ndarray:
        """Local block id (slot * k + half * k/2 + j) -> physical block id."""
        hk = k // 2
        t = np.empty(2 * k, dtype=np.int32)
        for s in range(2):
            for h in range(2):
                t[s * k + h * hk:s * k + (h + 1) * hk] = self.loc[s][h] * hk + np.arange(hk)
        return t

    def moves_to_canonical(self) -> list:
        """(src buffer, dst buffer) copies that bring (slot, half) back to
        buffer 2 slot + half, using the spare as scratch (applied in order)."""
        mv = []
        if self.spare is None:
            return mv
        for h in range(2):
            where = {0: self.loc[0][h], 1: self.loc[1][h]}  # slot -> buffer
            free = self.spare[h]
            for _ in range(4):
                todo = [s for s in (0, 1) if where[s] != 2 * s + h]
                if not todo:
                    break
                ready = [s for s in todo if 2 * s + h == free]
                if ready:
                    s = ready[0]
                    mv.append((where[s], free))
                    where[s], free = free, where[s]
                else:  # both slots sit in each other's home: park one in the spare
                    s = todo[0]
                    mv.append((where[s], free))
                    where[s], free = free, where[s]
            self.loc[0][h], self.loc[1][h], self.spare[h] = where[0], where[1], free
        return mv


def advance_placement(tour, r: int, phys: list) -> None:
    """Round r's exchange applied to ``phys`` in place (phys[h][s] = the
    super-block resident in slot s of GPU h; every rank keeps the whole
    table, exchanges are deterministic): GPU h's slot xslot[r][h] now holds
    what its source held in the slot that one gave up."""
    old = [list(p) for p in phys]
    for h in range(len(phys)):
        src = int(tour.recv_from[r, h])
        phys[h][int(tour.xslot[r, h])] = old[src][int(tour.xslot[r, src])]
