#!/usr/bin/env python3
"""CPU only (numpy): the queueing rule of the packed walk (walk_list_packed / walk_ring_drain in csrc/nms_kernels.hpp) replayed on
one frame of the bench's box recipe, to COUNT what a list's sequential chain is made of -- not to time it and not to test the kernel.

    python devtools/walk_filter_sim.py [--boxes 10000] [--thresh 0.3] [--orders 3] [--canvas 1.0]

Today's rule: chunks of 64 candidates in list order; a candidate whose dead bit is clear at the start of its chunk's pass is
queued in a ring; while the ring holds eight candidates (at the end of the list: any) a group of eight is taken, a member is
tested again when its group starts ("dead member" if it died in between), the survivors of the group -- greedy inside the group --
OR their adjacency lists into the dead mask.
Wide rule (what walk_list_packed's tail does): after the first narrow pass that queued at most NSW candidates the list is taken
W chunks per pass.  Stage 1, one pass AHEAD (i.e. before the previous block's groups ran): the W x 64 ids are tested and the
wanted ones compacted in list order; more than 64 of them -> the block is an OVERFLOW block.  Stage 2, in the block's own pass:
the compacted candidates are tested again, the alive ones queued, the ring drained.  An overflow block is queued slice by slice
(64 ids, fresh test, drain) instead.
Printed per rule and order: filter passes, groups, candidates queued, survivors, members found dead at group start, the ring's
high-water mark, and for the wide rules where the switch happened and how many blocks overflowed."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import synth  # noqa: E402


def adjacency(b, t):
    """neighbour lists under the reference's rule: inter / union >= t with the + 1 pixel convention, float32 boxes in float64."""
    b = b.astype(np.float64)
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    adj = []
    for r0 in range(0, len(b), 1000):
        r = b[r0:r0 + 1000]
        w = np.minimum(r[:, None, 2], b[None, :, 2]) - np.maximum(r[:, None, 0], b[None, :, 0]) + 1
        h = np.minimum(r[:, None, 3], b[None, :, 3]) - np.maximum(r[:, None, 1], b[None, :, 1]) + 1
        inter = np.maximum(w, 0) * np.maximum(h, 0)
        hit = inter >= t * (area[r0:r0 + 1000, None] + area[None, :] - inter)
        hit[np.arange(len(r)), r0 + np.arange(len(r))] = False
        adj.extend(np.flatnonzero(row) for row in hit)
    return adj


class Walk:
    def __init__(self, adj, n):
        self.adj, self.dead, self.ring = adj, np.zeros(n, bool), []
        self.passes = self.groups = self.queued = self.kept = self.dead_members = self.high = self.overflow = 0
        self.switch_at = -1

    def queue(self, ids):
        ids = [c for c in ids if not self.dead[c]]
        self.ring.extend(ids)
        self.queued += len(ids)
        self.high = max(self.high, len(self.ring))

    def drain(self, flush):
        while len(self.ring) >= 8 or (flush and self.ring):
            grp, self.ring = self.ring[:8], self.ring[8:]
            self.groups += 1
            live = [c for c in grp if not self.dead[c]]
            self.dead_members += len(grp) - len(live)
            surv = []
            for c in live:                                     # greedy inside the group: an earlier SURVIVING member wins
                if not any(c in self.adj_set(s) for s in surv):
                    surv.append(c)
            for s in surv:
                self.dead[self.adj[s]] = True
            self.kept += len(surv)

    def adj_set(self, s):
        return set(self.adj[s].tolist())


def walk(adj, order, W=1, nsw=-1):
    """W = 1: today's rule.  W > 1: wide after the first narrow pass (not the list's first) that queued <= nsw candidates."""
    n = len(order)
    wk = Walk(adj, len(adj))
    q = 0
    while q < n:
        before = wk.queued
        wk.passes += 1
        wk.queue(order[q:q + 64])
        wk.drain(q + 64 >= n)
        q += 64
        if W > 1 and q > 64 and q < n and wk.queued - before <= nsw:
            wk.switch_at = q
            break
    if q < n and W > 1:
        span = 64 * W
        want = [c for c in order[q:q + span] if not wk.dead[c]]                     # stage 1 of the first block (prologue)
        while q < n:
            nxt = [c for c in order[q + span:q + 2 * span] if not wk.dead[c]]      # stage 1 of the next block, one pass ahead
            wk.passes += 1
            if len(want) <= 64:
                wk.queue(want)
                wk.drain(q + span >= n)
            else:
                wk.overflow += 1
                for s in range(q, min(q + span, n), 64):
                    wk.queue(order[s:s + 64])
                    wk.drain(s + 64 >= n)
            q += span
            want = nxt
    return wk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boxes", type=int, default=10000)
    ap.add_argument("--thresh", type=float, default=0.3)
    ap.add_argument("--orders", type=int, default=3)
    ap.add_argument("--canvas", type=float, default=1.0, help="shrink the recipe's canvas (denser frames)")
    ap.add_argument("--seed", type=int, default=2000)
    a = ap.parse_args()
    rng = np.random.RandomState(a.seed)
    b = synth.boxes_1(rng, a.boxes)
    if a.canvas != 1.0:
        b[:, [0, 2]] *= a.canvas
        b[:, [1, 3]] *= a.canvas
        b = np.round(b)
    adj = adjacency(b, a.thresh)
    print("boxes %d  threshold %.2f  average degree %.1f" % (a.boxes, a.thresh, np.mean([len(x) for x in adj])))
    rules = [("today", 1, -1)] + [("W=%d nsw=%d" % (W, nsw), W, nsw) for W in (4, 8) for nsw in (8, 12, 16, 24)]
    print("%-14s %5s %6s %6s %6s %6s %5s %5s %7s %5s" % ("rule", "order", "passes", "groups", "queued", "kept", "dead", "ring", "switch", "ovfl"))
    ref = None
    for name, W, nsw in rules:
        for o in range(a.orders):
            order = np.random.RandomState(a.seed + 1 + o).permutation(a.boxes)
            wk = walk(adj, order, W, nsw)
            if W == 1:
                ref = ref or {}
                ref[o] = wk.kept
            assert wk.kept == ref[o], "the wide rule changed the result"
            print("%-14s %5d %6d %6d %6d %6d %5d %5d %7d %5d" % (name, o, wk.passes, wk.groups, wk.queued, wk.kept, wk.dead_members, wk.high,
                                                                   wk.switch_at, wk.overflow))


if __name__ == "__main__":
    main()
