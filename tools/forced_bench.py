#!/usr/bin/env python3
"""Forced playouts and policy target pruning at the root (fpc_search_set_forced, args["forced_playouts"]): what does the
pair cost per simulation step, and what does it do to the root's visit counts and to the policy target?

    python3 tools/forced_bench.py --out DIR [--slots 256] [--sims 400] [--repeats 3] [--factor 2.0]

One ply from the start position (G times) and one from tools/refill_bench.py's near-end positions, with the same network
(ResNet(blocks, hidden), seeded random weights, fp16), under FPC_RULES_SELFPLAY (63) with first-play urgency and root
Dirichlet noise (alpha 0.3, eps 0.25, the same draws in both arms) on, factor 0 then `factor` alternating on ONE engine,
`repeats` times after an untimed warm-up of both arms.  Per position set and arm:
  * ms_per_step: fpc_search_begin, then fpc_search_run(sims) and fpc_search_results between device synchronisations, and
    the fpc_stats stage times per step of the same runs (fpc_set_timing is on in both arms alike);
  * visited_children: the root children with N > 0;
  * pruned_share: the share of the root's child visits that fpc_search_targets leaves out (0 in the factor-0 arm, where
    the targets are the stored counts), pruned_to_zero: the children with N > 0 whose target is 0, per game;
  * pv_depth: the depth of the tree along its most-visited line (tools/visits_bench.py's: the finished search is re-rooted
    on the most-visited root child until the root has no child).
DIR/forced_bench.json holds one JSON record (also printed)."""
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
from visits_bench import pv_depth, quantiles

RULES = fpc_ffi.RULES_SELFPLAY


def timed_ply(eng, pods, sims, factor, fpu, gamma):
    eng.set_rule_bits(RULES)
    eng.set_fpu(fpc_ffi.FPU_PARENT, fpu)
    eng.set_root_noise(gamma, 0.25)
    eng.set_forced(factor)
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


def describe(eng, res):
    """the root's counts and the targets of the finished search, per game with children"""
    tgt = eng.search_targets()
    visited, share, to_zero = [], [], []
    for g in range(len(res["root_n"])):
        n = int(res["n_children"][g])
        if n == 0:
            continue
        vis, t = res["visits"][g, :n].astype(np.int64), tgt[g, :n].astype(np.int64)
        visited.append(int((vis > 0).sum()))
        share.append(float((vis - t).sum()) / float(max(vis.sum(), 1)))
        to_zero.append(int(((vis > 0) & (t == 0)).sum()))
    return {"sims_done": quantiles(res["sims_done"]), "visited_children": quantiles(visited), "pruned_share": quantiles(share),
            "pruned_to_zero": quantiles(to_zero)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--factor", type=float, default=2.0)
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
    arms = (("factor0", 0.0), ("factor%g" % a.factor, a.factor))
    torch.manual_seed(0)
    model = net.ResNet(Spec(R), a.blocks, a.hidden, "cpu").eval()
    eng = fpc_ffi.Engine(R, INV, max_games=G, max_sims=sims + 16, nn_dtype=1)
    eng.load_weights(weights.export_weights(model, 1))
    turn, entries = positions.start_entries(R)
    eng.set_rules(fpc_ffi.RULES_FIXED)                       # the playouts that make the near-end positions: full moves
    near, gen = start_positions(eng, G, a.playout, a.oversample, a.seed)
    sets = {"start": fpc_ffi.pods_of([fpc_ffi.board_from_dict(R, turn, entries)] * G), "near_end": near}
    gamma = np.random.default_rng(a.seed).standard_gamma(0.3, size=(G, fpc_ffi.MAX_MOVES)).astype(np.float32)
    for _, factor in arms:                                   # untimed: first launches, allocations, both arms once
        timed_ply(eng, sets["start"], min(sims, 16), factor, a.fpu, gamma)
    runs = []
    for rep in range(a.repeats):
        for where, pods in sets.items():
            for name, factor in arms:
                dt, res, st = timed_ply(eng, pods, sims, factor, a.fpu, gamma)
                fwd = max(int(st["launches_nn"]), 1)
                rec = {"arm": name, "positions": where, "repeat": rep, "search_s": dt, "ms_per_step": 1e3 * dt / sims,
                       "stage_ms_per_step": {"select+encode": st["ms_select"] / fwd, "tower": st["ms_tower"] / fwd,
                                             "policy_linear": st["ms_fc"] / fwd, "expand+backup": st["ms_expand"] / fwd}}
                if rep == 0:                                 # the trees are the same in every repeat
                    rec.update(describe(eng, res))
                    eng.set_root_noise(None, 0.0)            # the walk below re-roots; it needs no noise
                    rec["pv_depth"] = quantiles(pv_depth(eng, res))
                runs.append(rec)
                print(json.dumps(rec), file=sys.stderr, flush=True)
    summary = {}
    for where in sets:
        for name, _ in arms:
            mine = [r for r in runs if r["arm"] == name and r["positions"] == where]
            first = dict(mine[0])
            for k in ("repeat", "search_s", "ms_per_step", "stage_ms_per_step"):
                first.pop(k)
            first["ms_per_step"] = [r["ms_per_step"] for r in mine]
            first["ms_per_step_median"] = float(np.median(first["ms_per_step"]))
            first["stage_ms_per_step"] = {k: [r["stage_ms_per_step"][k] for r in mine] for k in mine[0]["stage_ms_per_step"]}
            summary["%s/%s" % (where, name)] = first
    out = {"tool": "forced_bench", "board": R, "blocks": a.blocks, "hidden": a.hidden, "slots": G, "sims": sims, "rules": RULES,
           "fpu": a.fpu, "factor": a.factor, "noise": {"alpha": 0.3, "eps": 0.25}, "repeats": a.repeats,
           "kernel": eng.L.fpc_nn_kernel(eng.h).decode(), "near_end_positions": gen, "summary": summary}
    eng.set_forced(0.0)
    eng.set_root_noise(None, 0.0)
    eng.close()
    line = json.dumps(out)
    print(line, flush=True)
    with open(os.path.join(a.out, "forced_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
