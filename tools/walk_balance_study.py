#!/usr/bin/env python3
"""How evenly the tiles of a slot load the waves of a k_walk_dg workgroup: a model on the CPU, no GPU needed.

`python tools/walk_balance_study.py [--graph webstanford] [--sources 24] [--sub 16] [--nw 8] [--tile 32 16] [--seg 1024 128]`

For the first `--sources` sources of the bench's query list the twin (tests/oracle_lib.py) pushes and counts the walks of
every node; the counts are cut into items of at most `--seg` walks in node order, the items into tiles of `--tile` items,
and the tiles dealt to `--sub` workgroups of `--nw` waves as the kernel deals them: tile t belongs to workgroup
(t / nw) % sub.  A wave's time is taken as proportional to its walks (its lanes are refilled every iteration, across
tiles).  Two hand-outs of a workgroup's tiles to its waves:
  static   wave w takes the workgroup's tiles w, w + nw, ... of its list (the stride the kernel had)
  ticket   the wave that is free first takes the workgroup's next tile (fora_consts.h: dg_ticket_tile)
A workgroup holds its LDS until its slowest wave ends, so the figure is the share of a slot's resident wave time that is
work: sum of wave work / (nw * slowest wave), summed over the slot's workgroups.  Printed: mean [min, max] over slots."""
import argparse
import heapq
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def tile_walks(cnt, seg, wt):
    """Walks per tile: per-node counts -> items of at most `seg` walks, node order -> tiles of `wt` items."""
    cnt = cnt[cnt > 0].astype(np.int64)
    nseg = (cnt + seg - 1) // seg
    first = np.cumsum(nseg) - nseg
    items = np.full(int(nseg.sum()), seg, dtype=np.int64)
    items[first + nseg - 1] = cnt - (nseg - 1) * seg   # a node's last item holds the rest
    pad = (-items.size) % wt
    return np.concatenate([items, np.zeros(pad, dtype=np.int64)]).reshape(-1, wt).sum(axis=1)


def efficiency(tiles, sub, nw, ticket):
    """Share of the slot's resident wave time that is work."""
    work = busy = 0
    for x in range(sub):
        mine = [int(tiles[t]) for t in range(tiles.size) if (t // nw) % sub == x]   # in ticket order
        if not mine:
            continue
        if ticket:
            waves = [0] * nw
            heapq.heapify(waves)
            for w in mine:
                heapq.heappush(waves, heapq.heappop(waves) + w)
        else:
            waves = [sum(mine[w::nw]) for w in range(nw)]
        work += sum(waves)
        busy += nw * max(waves)
    return work / busy if busy else 1.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--graph", default="webstanford")
    ap.add_argument("--dangling", default="none", choices=["none", "rmat"])
    ap.add_argument("--sources", type=int, default=24)
    ap.add_argument("--epsilon", type=float, default=0.5)
    ap.add_argument("--sub", type=int, default=16, help="workgroups per slot (1: option xb = 1)")
    ap.add_argument("--nw", type=int, nargs="+", default=[8], help="waves per workgroup")
    ap.add_argument("--tile", type=int, nargs="+", default=[32, 16], help="items per tile")
    ap.add_argument("--seg", type=int, nargs="+", default=[1024], help="walks per item at most")
    args = ap.parse_args()
    import oracle_lib as O
    from fora_amd import synth
    O.build()
    n, m, row_ptr, col = synth.preset(args.graph, args.dangling)
    g = O.Graph(n, m, row_ptr, col)
    rmax, omega = O.fora_setting(n, m, args.epsilon)
    counts = []
    for s in synth.query_set(n, 1000, 20261001)[:args.sources]:  # the bench's draw of 1000 sources, its first ones
        push = O.twin_push(g, int(s), rmax)
        if push["rsum_fix"]:
            counts.append(O.twin_walk_counts(g, push["residue"], push["rsum_fix"], omega)[1])
    print(f"{args.graph}: {len(counts)} slots with walks, {np.mean([int(c.sum()) for c in counts]):.0f} walks per slot, sub {args.sub}")
    print("  nw tile   seg  hand-out   work / resident wave time: mean [min, max]   tiles per slot")
    for nw in args.nw:
        for seg in args.seg:
            for wt in args.tile:
                tiles = [tile_walks(c, seg, wt) for c in counts]
                for name, ticket in (("static", False), ("ticket", True)):
                    e = [efficiency(t, args.sub, nw, ticket) for t in tiles]
                    print(f"  {nw:2d} {wt:4d} {seg:5d}  {name:8s}   {np.mean(e):.3f} [{min(e):.3f}, {max(e):.3f}]"
                          f"   {np.mean([t.size for t in tiles]):.0f}")


if __name__ == "__main__":
    main()
