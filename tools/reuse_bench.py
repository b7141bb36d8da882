#!/usr/bin/env python3
"""Subtree reuse (fpc_search_advance): what a ply keeps and what the advance costs.

    python3 tools/reuse_bench.py --out DIR [--plies 8] [--games 256] [--sims 400] [--only reuse]

Shape: BASELINE.json configs[1] -- ResNet(10,128), seeded random weights, 256 games x 400 simulations, 14x14, fp16 --
for eight plies of self-play, once with a fresh tree every ply (fpc_search_begin) and once with the played move's
subtree kept (fpc_search_advance, engine created with max_sims = 2 x sims; a ply runs min(sims, room under max_sims)
new simulations).  Moves are sampled from the root visit counts (temperature 1, seeded), finished games leave the batch.
Per ply: wall time of the begin / advance call including its read-back, wall time of the search that follows (between
device synchronisations), their ratio, and the distribution of kept_visits / sims.  DIR/fresh.json and DIR/reuse.json
hold one JSON record per arm (also printed).  --only ARM runs a single arm (e.g. under a kernel trace)."""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(HERE, "alphazero-4-player-chess_amd"), HERE]
import numpy as np
import torch

import fpc_ffi
import net
import positions
import selfplay
import weights
from bench import Spec


def run(arm, R, blocks, hidden, G, sims, plies, seed):
    INV = {8: 2, 14: 3}[R]
    reuse = arm == "reuse"
    torch.manual_seed(0)
    model = net.ResNet(Spec(R), blocks, hidden, "cpu").eval()
    eng = fpc_ffi.Engine(R, INV, max_games=G, max_sims=sims * (2 if reuse else 1), nn_dtype=1)
    eng.load_weights(weights.export_weights(model, 1))
    turn, entries = positions.start_entries(R)
    start = fpc_ffi.board_from_dict(R, turn, entries)
    pods = fpc_ffi.pods_of([start] * G)
    rng = np.random.default_rng(seed)
    per_ply = []
    keep, picks = None, None
    for ply in range(plies + 1):                         # ply 0 warms up (first launches, allocations) and is not reported
        n = pods.shape[0]
        if n == 0:
            break
        kept = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if reuse and ply > 0:
            pods = np.zeros((n, fpc_ffi.BOARD_BYTES), np.uint8)
            kept = eng.search_advance(picks, keep, roots_np=pods)
            run_sims = min(sims, eng.max_sims - (int(kept.max()) - 1))
        else:
            eng.search_begin_np(pods, 3.0)
            run_sims = sims
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        eng.search_run(run_sims)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        res = eng.search_results(roots_np=pods)
        flats = np.zeros(n, np.int32)
        for g in range(n):
            k = int(res["n_children"][g])
            flats[g] = selfplay.sample_action(res["flat"][g, :k], res["visits"][g, :k], 1.0, float(rng.random()))
        nxt = eng.take_action_np(pods, flats)
        over = eng.game_result_np(nxt) != 0
        keep = np.nonzero(~over)[0].astype(np.int32)
        picks = flats[keep]
        pods = np.ascontiguousarray(nxt[keep])
        if ply == 0:
            continue
        rec = {"ply": ply, "games": n, "sims_run": run_sims, "start_ms": 1e3 * (t1 - t0), "search_ms": 1e3 * (t2 - t1),
               "start_over_search": (t1 - t0) / (t2 - t1), "root_visits_mean": float(res["root_n"].mean())}
        if kept is not None:
            f = kept.astype(np.float64) / sims
            rec["kept_fraction"] = {"mean": float(f.mean()), "median": float(np.median(f)), "p10": float(np.percentile(f, 10)),
                                    "p90": float(np.percentile(f, 90)), "max": float(f.max())}
        per_ply.append(rec)
    kernel = eng.L.fpc_nn_kernel(eng.h).decode()
    eng.close()
    return {"arm": arm, "board": R, "blocks": blocks, "hidden": hidden, "games": G, "sims": sims, "plies": per_ply,
            "kernel": kernel, "start_call": "fpc_search_advance" if reuse else "fpc_search_begin"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--plies", type=int, default=8)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--board", type=int, default=14)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--only", default=None, choices=["fresh", "reuse"])
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    for arm in ([a.only] if a.only else ["fresh", "reuse"]):
        rec = run(arm, a.board, a.blocks, a.hidden, a.games, a.sims, a.plies, seed=7)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(os.path.join(a.out, "%s.json" % arm), "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
