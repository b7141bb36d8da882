#!/usr/bin/env python3
"""FPC_RULES_VISITS (fpc_set_rule_bits bit 32, args["rules"] = "selfplay") and first-play urgency (fpc_search_set_fpu,
args["fpu"]): what do they change in one ply of search, and what do they cost?

    python3 tools/visits_bench.py --out DIR [--slots 256] [--sims 400] [--repeats 3] [--fpu 0.25]

Searches the same G positions with the same network (ResNet(blocks, hidden), seeded random weights, fp16) for one ply of
`sims` simulations, once from the start position (G copies) and once from tools/refill_bench.py's near-end positions,
under three arms -- rules 31 (FPC_RULES_TRAINING), rules 63 (FPC_RULES_SELFPLAY), rules 63 with FPC_FPU_PARENT and the
given reduction -- alternating, `repeats` times, in one process after an untimed warm-up of every arm.  Per arm and set of
positions:
  * fpc_search_begin, then fpc_search_run(sims) between device synchronisations with stage timing on, as bench.py
    times its plies: the time per simulation step and the fpc_stats stage times per step;
  * root_visits: the simulations through the root at move time (root N minus the visit a root is born with);
  * phantom_pi_share: the share of the policy target pi = N / sum N that lies on root children with no real visit --
    under rules 31 the children still at their birth count of 1 over sum N, under rules 63 zero by construction;
  * visited_children: the root children with a real visit (N above the birth count), and the root's child count;
  * pv_depth: the depth of the tree along its most-visited line, read by re-rooting the finished search on the
    most-visited child (fpc_search_advance) until the root has no child.
DIR/visits_bench.json holds one JSON record (also printed)."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(HERE, "alphazero-4-player-chess_amd"), HERE, os.path.join(HERE, "tools")]
import numpy as np
import torch

import fpc_ffi
import net
import positions
import weights
from bench import Spec
from refill_bench import start_positions


def quantiles(x):
    x = np.asarray(x)
    return {"n": int(x.size), "min": float(x.min()), "p10": float(np.percentile(x, 10)), "median": float(np.median(x)),
            "mean": float(x.mean()), "p90": float(np.percentile(x, 90)), "max": float(x.max())}


def set_arm(eng, arm):
    eng.set_rule_bits(arm["rules"])
    if arm["fpu"] is None:
        eng.set_fpu(fpc_ffi.FPU_ZERO, 0.0)
    else:
        eng.set_fpu(fpc_ffi.FPU_PARENT, arm["fpu"])


def timed_ply(eng, arm, pods, sims):
    set_arm(eng, arm)
    eng.search_begin_np(pods, 3.0)
    eng.stats_reset()
    eng.set_timing(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.search_run(sims)
    res = eng.search_results()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    eng.set_timing(False)
    return dt, res, eng.stats()


def pv_depth(eng, res):
    """levels below the root along the most-visited line of every game: advances until the root has no child"""
    G = len(res["root_n"])
    depth = np.zeros(G, np.int64)
    games = np.arange(G)                                     # the original game of every row of the current search
    while True:
        n = res["n_children"]
        keep = np.nonzero(n > 0)[0]
        if keep.size == 0:
            return depth
        depth[games[keep]] += 1
        flats = [int(res["flat"][g, int(np.argmax(res["visits"][g, :n[g]]))]) for g in keep]
        eng.search_advance(flats, keep.astype(np.int32))
        games = games[keep]
        res = eng.search_results()


def describe(res, born):
    G = len(res["root_n"])
    share, visited, children = [], [], []
    for g in range(G):
        n = int(res["n_children"][g])
        if n == 0:
            continue
        vis = res["visits"][g, :n].astype(np.int64)
        share.append(float(((vis == born) * vis).sum()) / float(max(vis.sum(), 1)))
        visited.append(int((vis > born).sum()))
        children.append(n)
    return {"root_visits": quantiles(res["root_n"] - born), "sims_done": quantiles(res["sims_done"]),
            "phantom_pi_share": quantiles(share), "visited_children": quantiles(visited), "children": quantiles(children)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--fpu", type=float, default=0.25)
    ap.add_argument("--board", type=int, default=14)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--playout", type=int, default=800)
    ap.add_argument("--oversample", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    R, G, sims = a.board, a.slots, a.sims
    INV = {8: 2, 14: 3}[R]
    arms = [{"name": "rules31", "rules": fpc_ffi.RULES_TRAINING, "fpu": None},
            {"name": "rules63", "rules": fpc_ffi.RULES_SELFPLAY, "fpu": None},
            {"name": "rules63_fpu", "rules": fpc_ffi.RULES_SELFPLAY, "fpu": a.fpu}]
    torch.manual_seed(0)
    model = net.ResNet(Spec(R), a.blocks, a.hidden, "cpu").eval()
    eng = fpc_ffi.Engine(R, INV, max_games=G, max_sims=sims + 16, nn_dtype=1)
    eng.load_weights(weights.export_weights(model, 1))
    turn, entries = positions.start_entries(R)
    eng.set_rules(fpc_ffi.RULES_FIXED)                       # the playouts that make the near-end positions: full moves
    near, gen = start_positions(eng, G, a.playout, a.oversample, a.seed)
    sets = {"start": fpc_ffi.pods_of([fpc_ffi.board_from_dict(R, turn, entries)] * G), "near_end": near}
    for arm in arms:                                         # untimed: first launches, allocations, every arm once
        timed_ply(eng, arm, sets["start"], min(sims, 16))
    runs = []
    for rep in range(a.repeats):
        for where, pods in sets.items():
            for arm in arms:
                dt, res, st = timed_ply(eng, arm, pods, sims)
                fwd = max(int(st["launches_nn"]), 1)
                born = 0 if arm["rules"] & fpc_ffi.RULES_VISITS else 1
                rec = {"arm": arm["name"], "positions": where, "repeat": rep, "search_s": dt, "ms_per_step": 1e3 * dt / sims,
                       "stage_ms_per_step": {"select+encode": st["ms_select"] / fwd, "tower": st["ms_tower"] / fwd,
                                             "policy_linear": st["ms_fc"] / fwd, "expand+backup": st["ms_expand"] / fwd}}
                if rep == 0:                                 # the trees are the same in every repeat
                    rec.update(describe(res, born))
                    rec["pv_depth"] = quantiles(pv_depth(eng, res))
                runs.append(rec)
                print(json.dumps(rec), file=sys.stderr, flush=True)
    summary = {}
    for where in sets:
        for arm in arms:
            mine = [r for r in runs if r["arm"] == arm["name"] and r["positions"] == where]
            first = dict(mine[0])
            for k in ("repeat", "search_s", "ms_per_step", "stage_ms_per_step"):
                first.pop(k)
            first["ms_per_step"] = [r["ms_per_step"] for r in mine]
            first["ms_per_step_median"] = float(np.median(first["ms_per_step"]))
            first["stage_ms_per_step"] = {k: [r["stage_ms_per_step"][k] for r in mine] for k in mine[0]["stage_ms_per_step"]}
            summary["%s/%s" % (where, arm["name"])] = first
    out = {"tool": "visits_bench", "board": R, "blocks": a.blocks, "hidden": a.hidden, "slots": G, "sims": sims, "fpu": a.fpu,
           "repeats": a.repeats, "kernel": eng.L.fpc_nn_kernel(eng.h).decode(), "near_end_positions": gen, "summary": summary}
    eng.close()
    line = json.dumps(out)
    print(line, flush=True)
    with open(os.path.join(a.out, "visits_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
