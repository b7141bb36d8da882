#!/usr/bin/env python3
"""Leaf-parallel search (fpc_search_set_leaves) throughput: simulations/s and ms per simulation step through the fused
loop (fpc_search_run), K leaves per game per step.

    python3 tools/leaves_bench.py --out DIR [--reps 5] [--only ref:2]

Arms: K = 1, 2, 3, 4 at the reference's shipped default (ResNet(15,256), seeded random weights, 100 games x 50 sims,
8x8) and K = 1, 2 at BASELINE.json configs[1] (ResNet(10,128), 256 games x 400 sims, 14x14); fp16.  Per config one
engine with K_max x G rows; every arm is warmed up first, then the arms are alternated rep by rep in this one process,
each search timed between device synchronisations.  One JSON line per arm goes to DIR/<config>_k<K>.json (and to
stdout): sims/s = leaf evaluations + terminal backups per second (sims_done summed over the games), ms/step = search
time / ceil(sims / K).  --only CONFIG:K runs a single arm (e.g. under a kernel trace)."""
import argparse
import json
import math
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
import weights
from bench import Spec

CONFIGS = {   # name: (board, blocks, hidden, games, sims, leaves)
    "ref": (8, 15, 256, 100, 50, (1, 2, 3, 4)),
    "c1": (14, 10, 128, 256, 400, (1, 2)),
}


def roots_for(eng, R, G, seed=7):
    """the start position advanced by 0..5 random legal plies per game (mixed sides to move)"""
    turn, entries = positions.start_entries(R)
    start = fpc_ffi.board_from_dict(R, turn, entries)
    rng = np.random.default_rng(seed)
    out = []
    for g in range(G):
        b = fpc_ffi.clone_board(start)
        for _ in range(g % 6):
            lm = eng.legal_moves([b])[0]
            b = eng.take_action([b], [lm[int(rng.integers(len(lm)))][2]])[0]
        out.append(b)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=None, help="CONFIG:K, e.g. ref:2")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    plan = {name: list(cfg[5]) for name, cfg in CONFIGS.items()}
    if a.only:
        name, k = a.only.split(":")
        plan = {name: [int(k)]}
    for name, ks in plan.items():
        R, blocks, hidden, G, sims, _ = CONFIGS[name]
        INV = {8: 2, 14: 3}[R]
        torch.manual_seed(0)
        model = net.ResNet(Spec(R), blocks, hidden, "cpu").eval()
        eng = fpc_ffi.Engine(R, INV, max_games=G * max(ks), max_sims=sims, nn_dtype=1)
        eng.load_weights(weights.export_weights(model, 1))
        roots0 = roots_for(eng, R, G)

        def one(k):
            eng.set_leaves(k)
            roots = [fpc_ffi.clone_board(b) for b in roots0]
            eng.search_begin(roots, 3.0)
            torch.cuda.synchronize()
            t = time.perf_counter()
            eng.search_run(sims)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t
            res = eng.search_results(roots=roots)
            return dt, int(res["sims_done"].sum())

        for k in ks:                                     # warm-up: first launches, allocations, code objects
            one(k)
        times = {k: [] for k in ks}
        done = {k: 0 for k in ks}
        for _ in range(a.reps):
            for k in ks:                                 # arms alternated rep by rep
                dt, n = one(k)
                times[k].append(dt)
                done[k] = n
        kernel = eng.L.fpc_nn_kernel(eng.h).decode()
        eng.close()
        for k in ks:
            dt = float(np.median(times[k]))
            steps = math.ceil(sims / k)
            rec = {"config": name, "leaves": k, "virtual_loss": 1.0, "board": R, "blocks": blocks, "hidden": hidden,
                   "games": G, "sims": sims, "steps": steps, "sims_done": done[k], "median_s": dt,
                   "sims_per_s": done[k] / dt, "ms_per_step": 1e3 * dt / steps, "reps_s": times[k],
                   "kernel": kernel}
            line = json.dumps(rec)
            print(line, flush=True)
            with open(os.path.join(a.out, "%s_k%d.json" % (name, k)), "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
