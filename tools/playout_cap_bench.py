#!/usr/bin/env python3
"""Playout cap randomization (fpc_search_set_fast_rows, args["playout_cap"]): what does drawing a fast search for most plies
change in self-play -- games, plies and full-search training records per second -- and are the budget-idle rows of a mixed
batch cheap enough for it to pay?

    python3 tools/playout_cap_bench.py --out DIR [--sims 400] [--length 8] [--repeats 3] [--full-prob 0.25]

Self-play from the start position on the headline network (ResNet(blocks, hidden), seeded random weights, fp16) under
rules = "selfplay" (63) with fpu 0.25, root Dirichlet noise (alpha 0.3, eps 0.25), forced_playouts 2, subtree reuse,
refill (2 x slots games over `slots` positions, every game `length` plies), device-side move choice, live-row numbering
and sim_budget "per_game".  Three arms alternate, `repeats` times, in one process after an untimed warm-up of every arm:
    off_256   no cap: every ply is a full search of `sims` simulations, 256 slots (the yardstick)
    cap_256   cap on: a ply is full with probability `full_prob`, else a fast search of sims / 4 simulations with an
              all-zero noise row and the fast-row mask, 256 slots
    cap_512   the same at 512 slots
A mixed batch still runs max(budget) steps: the fast rows are idle (dead rows, which live-row numbering keeps out of the
network) once their budget is spent.  Per arm: games/s, plies/s, full-search records/s (the plies whose policy target is
trained), live rows per step (simulations completed / steps run), the fpc_stats stage times per step (fpc_set_timing is
on in every arm alike), the search's wall time per ply.  The summary gives the medians and their ratios to off_256.
DIR/playout_cap_bench.json holds one JSON record (also printed)."""
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
import selfplay
import weights
from bench import Spec
from mcts import budgets_for

RULES = fpc_ffi.RULES_SELFPLAY
ARMS = (("off_256", 256, False), ("cap_256", 256, True), ("cap_512", 512, True))
STAGES = ("ms_select", "ms_tower", "ms_fc", "ms_expand")


def run_arm(eng, name, G, boards, sims, fast_sims, full_prob, cap, args, uniforms, cap_uniforms, seed):
    rng = np.random.default_rng(seed)
    log = {"search_s": [], "steps": 0, "fast_plies": 0, "full_plies": 0}
    eng.set_rule_bits(RULES)
    eng.set_fpu(fpc_ffi.FPU_PARENT, 0.25)
    eng.set_forced(2.0)

    def ply(pods, kept, fast):
        """the search of one ply on the trees just begun or advanced; fast: one bool per game or None"""
        eng.set_live_rows(True)
        if fast is not None:
            eng.search_set_fast_rows(fast)
        budget = budgets_for(kept, sims, eng.max_sims, "per_game", 0, fast=fast, fast_searches=fast_sims if fast is not None else None)
        eng.search_set_budget(budget)
        run = max(budget)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.search_run(run)
        res = eng.search_results(roots=pods)
        torch.cuda.synchronize()
        log["search_s"].append(time.perf_counter() - t0)
        log["steps"] += run
        n_fast = int(sum(fast)) if fast is not None else 0
        log["fast_plies"] += n_fast
        log["full_plies"] += len(pods) - n_fast
        return res

    def noise(n, fast):
        gamma = rng.standard_gamma(0.3, size=(n, fpc_ffi.MAX_MOVES)).astype(np.float32)
        if fast is not None:
            gamma[np.asarray(fast, bool)] = 0.0              # a fast row keeps its priors un-noised
        eng.set_root_noise(gamma, 0.25)

    def search_fn(pods, fast=None):
        noise(len(pods), fast)
        eng.search_begin(pods, 3.0)
        return ply(pods, [0] * len(pods), fast)

    def continue_fn(keep_idx, picks, pods, fast=None):
        noise(len(pods), fast)
        if any(k < 0 for k in keep_idx):
            kept = eng.search_advance_refill(picks, keep_idx, fresh=pods, roots=pods)
        else:
            kept = eng.search_advance(picks, keep_idx, roots=pods)
        return ply(pods, kept, fast)

    eng.stats_reset()
    eng.set_timing(True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eps = selfplay.play(search_fn, eng, boards[:G], args, uniforms, continue_fn=continue_fn, refill=boards[G:], device_play=True,
                        playout_cap={"full_prob": full_prob, "fast_searches": fast_sims} if cap else None,
                        cap_uniforms=cap_uniforms if cap else None)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    eng.set_timing(False)
    st = eng.stats()
    plies = int(sum(e.length for e in eps))
    assert plies == log["fast_plies"] + log["full_plies"]
    fwd = max(int(st["launches_nn"]), 1)
    return {"arm": name, "slots": G, "seconds": dt, "games": len(eps), "games_per_s": len(eps) / dt, "plies": plies,
            "plies_per_s": plies / dt, "full_plies": log["full_plies"], "fast_plies": log["fast_plies"],
            "full_records_per_s": log["full_plies"] / dt, "searches": len(log["search_s"]), "steps": log["steps"],
            "sims_completed": int(st["sims"]), "live_rows_per_step": float(st["sims"]) / max(log["steps"], 1),
            "network_forwards": int(st["launches_nn"]),
            "stage_ms_per_step": {k[3:]: st[k] / fwd for k in STAGES},
            "search_s_total": float(np.sum(log["search_s"])), "search_ms_per_ply": 1e3 * float(np.sum(log["search_s"])) / plies,
            "search_ms_per_batch_ply": 1e3 * float(np.mean(log["search_s"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--length", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--full-prob", type=float, default=0.25)
    ap.add_argument("--board", type=int, default=14)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    R, L, sims = a.board, a.length, a.sims
    fast_sims = max(sims // 4, 1)
    INV = {8: 2, 14: 3}[R]
    torch.manual_seed(0)
    model = net.ResNet(Spec(R), a.blocks, a.hidden, "cpu").eval()
    blob = weights.export_weights(model, 1)
    engines = {}
    for G in sorted({g for _, g, _ in ARMS}):
        engines[G] = fpc_ffi.Engine(R, INV, max_games=G, max_sims=2 * sims, nn_dtype=1)
        engines[G].load_weights(blob)
    turn, entries = positions.start_entries(R)
    start = fpc_ffi.board_from_dict(R, turn, entries)
    Mmax = 2 * max(g for _, g, _ in ARMS)
    args = {"temperature": 1.0, "max_game_length": L, "heuristic_weight": 0.02}
    uniforms = np.random.default_rng(a.seed + 1).random((L, Mmax)).tolist()
    cap_uniforms = np.random.default_rng(a.seed + 2).random((L, Mmax)).tolist()

    def arm(name, G, cap, length, games):
        boards = [fpc_ffi.clone_board(start) for _ in range(games)]
        return run_arm(engines[G], name, G, boards, sims, fast_sims, a.full_prob, cap, dict(args, max_game_length=length), uniforms,
                       cap_uniforms, a.seed + 3)

    for name, G, cap in ARMS:                                # untimed: first launches, allocations, every path once
        arm(name, G, cap, 2, G + 8)
    runs = []
    for rep in range(a.repeats):
        for name, G, cap in ARMS:
            rec = arm(name, G, cap, L, 2 * G)
            rec["repeat"] = rep
            runs.append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)
    keys = ("games_per_s", "plies_per_s", "full_records_per_s", "live_rows_per_step", "search_ms_per_ply", "search_ms_per_batch_ply")
    summary = {}
    for name, G, cap in ARMS:
        mine = [r for r in runs if r["arm"] == name]
        s = {"slots": G, "cap": cap, "games": mine[0]["games"], "plies": mine[0]["plies"], "full_plies": mine[0]["full_plies"],
             "fast_plies": mine[0]["fast_plies"], "steps": mine[0]["steps"]}
        for k in keys:
            s[k] = [r[k] for r in mine]
            s[k + "_median"] = float(np.median(s[k]))
        s["stage_ms_per_step_median"] = {k: float(np.median([r["stage_ms_per_step"][k] for r in mine])) for k in mine[0]["stage_ms_per_step"]}
        summary[name] = s
    base = summary[ARMS[0][0]]
    for name, _, _ in ARMS:
        summary[name]["ratio_to_" + ARMS[0][0]] = {k: summary[name][k + "_median"] / base[k + "_median"] for k in keys}
    spread = {name: {k: (max(summary[name][k]) - min(summary[name][k])) / summary[name][k + "_median"] for k in ("games_per_s", "full_records_per_s")}
              for name, _, _ in ARMS}
    kernel = engines[256].L.fpc_nn_kernel(engines[256].h).decode()
    out = {"tool": "playout_cap_bench", "board": R, "blocks": a.blocks, "hidden": a.hidden, "sims": sims, "fast_sims": fast_sims,
           "full_prob": a.full_prob, "max_game_length": L, "repeats": a.repeats, "rules": RULES, "fpu": 0.25, "forced": 2.0,
           "noise": {"alpha": 0.3, "eps": 0.25}, "kernel": kernel, "summary": summary,
           "spread_max_minus_min_over_median": spread, "runs": runs}
    for eng in engines.values():
        eng.set_forced(0.0)
        eng.set_root_noise(None, 0.0)
        eng.close()
    line = json.dumps(out)
    print(line, flush=True)
    with open(os.path.join(a.out, "playout_cap_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
