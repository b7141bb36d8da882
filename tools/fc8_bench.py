#!/usr/bin/env python3
"""Opt-in int8 weights for the policy Linear (args["fc_weights"] = "int8", k_fcw8): what does halving the Linear's weight
stream buy on the headline shape?

    python3 tools/fc8_bench.py --out DIR [--sims 400] [--rounds 3]

Two engines in one process, built from the same torch module (ResNet(blocks, hidden), seeded random weights, fp16, full
policy head, `games` start positions): arm "w16" is the default code path (k_fcw) and the yardstick, arm "int8" runs
k_fcw8.  After an untimed warm-up of both, the arms alternate w16 int8 w16 int8 ... for `rounds` rounds; each run is one
ply of `sims` simulations (fpc_search_begin, then fpc_search_run between device synchronisations, fpc_set_timing on).
Per arm: median and range over the rounds of ms_fc (policy Linear + split-K reduce) and ms_tower per step, the step time,
the simulations per second, and the device memory the engine took (free memory before its creation minus after its load).
"speedup_condition_met": the int8 arm's median ms_fc lies below the w16 arm's by more than the w16 arm's own range.
DIR/fc8_bench.json holds one JSON record (also printed)."""
import argparse
import json
import os
import socket
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(HERE, "alphazero-4-player-chess_amd"), HERE, os.path.join(HERE, "tools")]
import numpy as np
import torch

import fpc_ffi
import net
import positions
from bench import Spec

ARMS = ("w16", "int8")
STAGES = ("ms_select", "ms_tower", "ms_fc", "ms_expand")


def timed_ply(eng, roots, sims):
    eng.search_begin([fpc_ffi.clone_board(b) for b in roots], 3.0)
    eng.stats_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.search_run(sims)
    res = eng.search_results()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, res, eng.stats()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--sims", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--board", type=int, default=14)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=128)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    R, sims = a.board, a.sims
    INV = {8: 2, 14: 3}[R]
    torch.manual_seed(0)
    model = net.ResNet(Spec(R), a.blocks, a.hidden, "cpu").eval().cuda()
    turn, entries = positions.start_entries(R)
    roots = [fpc_ffi.board_from_dict(R, turn, entries) for _ in range(a.games)]
    engs, mem = {}, {}
    first = fpc_ffi.Engine(R, INV, max_games=1, max_sims=1, nn_dtype=1)      # the process's one-time device allocations
    for arm in ARMS:
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        engs[arm] = fpc_ffi.Engine(R, INV, max_games=a.games, max_sims=sims, nn_dtype=1)
        engs[arm].load_weights_device(model, fc_weights=arm)
        engs[arm].set_timing(True)
        torch.cuda.synchronize()
        mem[arm] = int(free0 - torch.cuda.mem_get_info()[0])
    first.close()
    kernels = {arm: engs[arm].nn_fc_kernel() for arm in ARMS}
    assert kernels["int8"] == "k_fcw8" and kernels["w16"] != "k_fcw8", kernels
    for arm in ARMS:                                         # untimed: first launches, every path once
        timed_ply(engs[arm], roots, min(sims, 16))
    runs = []
    for rnd in range(a.rounds):
        for arm in ARMS:
            dt, res, st = timed_ply(engs[arm], roots, sims)
            rec = {"arm": arm, "round": rnd, "search_s": dt, "ms_per_step": 1e3 * dt / sims,
                   "sims_done": int(res["sims_done"].sum()), "sims_per_s": float(res["sims_done"].sum()) / dt}
            rec.update({k + "_per_step": st[k] / sims for k in STAGES})
            runs.append(rec)
            print(json.dumps(rec), file=sys.stderr, flush=True)
    summary = {}
    for arm in ARMS:
        mine = [r for r in runs if r["arm"] == arm]
        summary[arm] = {"fc_kernel": kernels[arm], "engine_device_bytes": mem[arm]}
        for k in ("ms_fc_per_step", "ms_tower_per_step", "ms_per_step", "sims_per_s"):
            v = [r[k] for r in mine]
            summary[arm][k] = {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v)), "runs": v}
    w, q = summary["w16"]["ms_fc_per_step"], summary["int8"]["ms_fc_per_step"]
    out = {"tool": "fc8_bench", "box": {"host": socket.gethostname(), "device": torch.cuda.get_device_name(0)},
           "board": R, "blocks": a.blocks, "hidden": a.hidden, "games": a.games, "sims": sims, "rounds": a.rounds,
           "tower_kernel": engs["w16"].L.fpc_nn_kernel(engs["w16"].h).decode(), "summary": summary,
           "ms_fc_gain": w["median"] - q["median"], "w16_ms_fc_range": w["max"] - w["min"],
           "speedup_condition_met": bool(w["median"] - q["median"] > w["max"] - w["min"]), "runs": runs}
    for e in engs.values():
        e.close()
    line = json.dumps(out)
    print(line, flush=True)
    with open(os.path.join(a.out, "fc8_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
