#!/usr/bin/env python3
"""Per-game simulation budgets (fpc_search_set_budget, args["sim_budget"]): what do they change in self-play with
subtree reuse and refill?

    python3 tools/budget_bench.py --out DIR [--games 512] [--slots 256] [--sims 400] [--length 12] [--repeats 3]

Plays the same M start positions (tools/refill_bench.py's: seeded random playouts cut a few plies before their end)
with the same network (ResNet(blocks, hidden), seeded random weights, fp16) as one refilled run of G slots with the
played move's subtree kept, three ways:
    reuse_tree    today: every ply runs min(sims, max_sims - (max kept - 1)) simulations for every game; max_sims = 2 x sims
    per_game      budget[g] = min(sims, max_sims - (kept[g] - 1)), max(budget) simulations run; max_sims = 2 x sims
    visit_target  budget[g] = max(0, sims - (kept[g] - 1)): every root is searched until `sims` simulations have gone
                  through it; max_sims = sims (half the node pool, board pool and second set of tree arrays)
The arms alternate, `repeats` times, in one process after an untimed warm-up of every path.  Per arm: simulations run
per ply (the step count of fpc_search_run), the distributions of sims_done and of root visits at move time for fresh and
kept rows separately, the search's wall time per ply (between device synchronisations), games and plies per second, and
the engine's device memory -- computed from the pool shapes, and the free-memory difference around fpc_create.
DIR/budget_bench.json holds one JSON record (also printed)."""
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
import selfplay
import weights
from bench import Spec
from mcts import budgets_for
from refill_bench import start_positions

ARMS = ("reuse_tree", "per_game", "visit_target")
NODE_BYTES = 4 + 8 + 4 + 2 + 4 + 4 + 2 + 4       # N, W, P, mv, parent, child0, nch, bslot
AVG_CHILDREN = 96                                 # fpc_create's default node pool: 1 + max_sims * 96 nodes per game


def tree_bytes(G, max_sims):
    """the tree side of one handle with subtree reuse in use: two sets of node arrays and board pools, the path buffer"""
    node_cap, board_cap = 1 + max_sims * AVG_CHILDREN, max_sims + 2
    return {"node_arrays_x2": 2 * G * node_cap * NODE_BYTES, "board_pools_x2": 2 * G * board_cap * fpc_ffi.BOARD_BYTES,
            "path": G * (max_sims + 2) * 4}


def quantiles(x):
    if len(x) == 0:
        return None
    x = np.asarray(x)
    return {"n": int(x.size), "min": int(x.min()), "p10": float(np.percentile(x, 10)), "median": float(np.median(x)),
            "mean": float(x.mean()), "p90": float(np.percentile(x, 90)), "max": int(x.max())}


def run_arm(eng, arm, boards, G, sims, args, uniforms):
    log = {"run": [], "search_s": [], "done_fresh": [], "done_kept": [], "visits_fresh": [], "visits_kept": [], "kept": []}

    def searched(kept, run, t0, res):
        torch.cuda.synchronize()
        log["search_s"].append(time.perf_counter() - t0)
        log["run"].append(run)
        fresh = np.asarray(kept) == 1
        log["done_fresh"] += res["sims_done"][fresh].tolist(); log["done_kept"] += res["sims_done"][~fresh].tolist()
        log["visits_fresh"] += (res["root_n"][fresh] - 1).tolist(); log["visits_kept"] += (res["root_n"][~fresh] - 1).tolist()
        log["kept"] += (np.asarray(kept)[~fresh] - 1).tolist()

    def search_fn(pods):
        eng.search_begin(pods, 3.0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.search_run(sims)
        res = eng.search_results(roots=pods)
        searched(np.ones(len(pods), np.int32), sims, t0, res)
        return res

    def continue_fn(keep_idx, picks, pods):
        if any(k < 0 for k in keep_idx):
            kept = eng.search_advance_refill(picks, keep_idx, fresh=pods, roots=pods)
        else:
            kept = eng.search_advance(picks, keep_idx, roots=pods)
        if arm == "reuse_tree":
            run = min(sims, eng.max_sims - (int(kept.max()) - 1))
        else:
            budget = budgets_for(kept, sims, eng.max_sims, arm)
            eng.search_set_budget(budget)
            run = max(budget)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.search_run(run)
        res = eng.search_results(roots=pods)
        searched(kept, run, t0, res)
        return res

    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eps = selfplay.play(search_fn, eng, boards[:G], args, uniforms, continue_fn=continue_fn, refill=boards[G:])
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    lengths = np.array([e.length for e in eps])
    return {"arm": arm, "max_sims": eng.max_sims, "seconds": dt, "games": len(eps), "games_per_s": len(eps) / dt,
            "plies": int(lengths.sum()), "plies_per_s": float(lengths.sum()) / dt, "searches": len(log["run"]),
            "sims_run_per_ply": quantiles(log["run"]), "search_s_per_ply_mean": float(np.mean(log["search_s"])),
            "search_s_total": float(np.sum(log["search_s"])),
            "sims_done_fresh": quantiles(log["done_fresh"]), "sims_done_kept": quantiles(log["done_kept"]),
            "root_visits_fresh": quantiles(log["visits_fresh"]), "root_visits_kept": quantiles(log["visits_kept"]),
            "kept_visits_at_advance": quantiles(log["kept"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--slots", type=int, default=256)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--length", type=int, default=12)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--board", type=int, default=14)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--playout", type=int, default=800)
    ap.add_argument("--oversample", type=int, default=5)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    R, G, M, L = a.board, a.slots, a.games, a.length
    INV = {8: 2, 14: 3}[R]
    torch.manual_seed(0)
    model = net.ResNet(Spec(R), a.blocks, a.hidden, "cpu").eval()
    blob = weights.export_weights(model, 1)
    torch.cuda.init()
    engines, created = {}, {}
    for max_sims in (2 * a.sims, a.sims):
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        eng = fpc_ffi.Engine(R, INV, max_games=G, max_sims=max_sims, nn_dtype=1)
        created[max_sims] = free0 - torch.cuda.mem_get_info()[0]        # what fpc_create itself allocates (no second tree set yet)
        eng.load_weights(blob)
        engines[max_sims] = eng
    eng_of = {"reuse_tree": engines[2 * a.sims], "per_game": engines[2 * a.sims], "visit_target": engines[a.sims]}
    pods, gen = start_positions(engines[a.sims], M, a.playout, a.oversample, a.seed)
    boards = [fpc_ffi.board_of(pods[i]) for i in range(M)]
    args = {"temperature": 1.0, "max_game_length": L, "heuristic_weight": 0.02}
    uniforms = np.random.default_rng(a.seed + 1).random((L, M)).tolist()
    warm = min(M, G + 8)
    free1 = torch.cuda.mem_get_info()[0]
    grown = {}
    for arm in ARMS:                                         # untimed: first launches, allocations, every path once
        run_arm(eng_of[arm], arm, boards[:warm], G, a.sims, dict(args, max_game_length=3), uniforms)
        torch.cuda.synchronize()
        free2 = torch.cuda.mem_get_info()[0]
        grown[arm], free1 = free1 - free2, free2             # the second tree set (and the budget array) of the arm's handle
    runs = []
    for rep in range(a.repeats):
        for arm in ARMS:
            rec = run_arm(eng_of[arm], arm, boards, G, a.sims, args, uniforms)
            rec["repeat"] = rep
            runs.append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)
    summary = {}
    for arm in ARMS:
        mine = [r for r in runs if r["arm"] == arm]
        ms = eng_of[arm].max_sims
        summary[arm] = {"max_sims": ms,
                        "games_per_s": [r["games_per_s"] for r in mine], "games_per_s_median": float(np.median([r["games_per_s"] for r in mine])),
                        "plies_per_s_median": float(np.median([r["plies_per_s"] for r in mine])),
                        "search_s_per_ply_mean": [r["search_s_per_ply_mean"] for r in mine],
                        "sims_run_per_ply": mine[0]["sims_run_per_ply"], "searches": mine[0]["searches"],
                        "sims_done_fresh": mine[0]["sims_done_fresh"], "sims_done_kept": mine[0]["sims_done_kept"],
                        "root_visits_fresh": mine[0]["root_visits_fresh"], "root_visits_kept": mine[0]["root_visits_kept"],
                        "kept_visits_at_advance": mine[0]["kept_visits_at_advance"],
                        "tree_bytes_from_pool_shapes": tree_bytes(G, ms), "tree_bytes_total": sum(tree_bytes(G, ms).values()),
                        "free_memory_drop_at_fpc_create": int(created[ms])}
    out = {"tool": "budget_bench", "board": R, "blocks": a.blocks, "hidden": a.hidden, "slots": G, "games": M, "sims": a.sims,
           "max_game_length": L, "repeats": a.repeats, "rules": "strict", "kernel": engines[a.sims].L.fpc_nn_kernel(engines[a.sims].h).decode(),
           "start_positions": gen, "free_memory_drop_in_warm_up": {k: int(v) for k, v in grown.items()}, "summary": summary, "runs": runs}
    for eng in engines.values():
        eng.close()
    line = json.dumps(out)
    print(line, flush=True)
    with open(os.path.join(a.out, "budget_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
