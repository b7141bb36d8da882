#!/usr/bin/env python3
"""Refreshing the engine's network from the live torch module: the host path against the device-side pack.

    python3 tools/weights_bench.py --out DIR [--blocks 10] [--hidden 128] [--repeats 7]

The module lies on the GPU (fp32), as it does in the training loop.  Per board -- 14x14 (the headline network,
ResNet(10,128), fp16) and 8x8 -- wall clock per refresh, every arm ending with the engine's stream synchronised:
  a_host      weights.export_weights + Engine.load_weights: download to the host, fold / permute / pad / round in torch on
              the CPU, upload, free and allocate the whole network again (what MCTS.sync_weights does without the opt-in);
  b_first     Engine.load_weights_device on a fresh engine: allocation as in a_host, then the pack kernels;
  c_inplace   Engine.load_weights_device on the loaded engine: the pack kernels write the live allocations.
In a further round with fpc_set_timing on: the HIP-event time of the pack kernels alone in c_inplace and the bandwidth
they reach on 4 A^2 + 2 Np Kp bytes (the policy Linear read as fp32 and written as 16-bit; the convolutions add ~1 %).
2 warm-up refreshes + `repeats` timed ones per arm (a_host: 1 + 3, it takes seconds), medians with min and max;
DIR/weights_bench.json holds one JSON record per board (also printed)."""
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
import weights
from bench import Spec

PEAK_GBS = 8000.0      # MI355X HBM3E


def spread(ms):
    a = np.asarray(ms, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()), "repeats": int(a.size)}


def timed(fn, warmup, repeats):
    out = []
    for it in range(warmup + repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        dt = 1e3 * (time.perf_counter() - t0)
        if it >= warmup:
            out.append(dt)
    return spread(out)


def run(R, blocks, hidden, repeats, dtype=1):
    INV = {8: 2, 14: 3}[R]
    torch.manual_seed(0)
    model = net.ResNet(Spec(R), blocks, hidden, "cuda").eval()
    eng = fpc_ffi.Engine(R, INV, max_games=256, max_sims=16, nn_dtype=dtype)
    A = eng.A
    layout = weights.default_fc_layout(R)
    gw = 384 if layout == 2 else 256
    Np, Kp = (A + gw - 1) // gw * gw, (A + 511) // 512 * 512
    rec = {"board": R, "net": "ResNet(%d,%d)" % (blocks, hidden), "dtype": "fp16" if dtype else "bf16", "fc_layout": layout,
           "A": A, "Np": Np, "Kp": Kp, "host_threads": torch.get_num_threads()}

    rec["a_host_ms"] = timed(lambda: eng.load_weights(weights.export_weights(model, dtype)), 1, 3)

    def first():
        e = fpc_ffi.Engine(R, INV, max_games=256, max_sims=16, nn_dtype=dtype)
        t0 = time.perf_counter()
        e.load_weights_device(model)
        dt = 1e3 * (time.perf_counter() - t0)
        e.close()
        return dt
    rec["b_first_ms"] = spread([first() for _ in range(3)])
    rec["c_inplace_ms"] = timed(lambda: eng.load_weights_device(model), 2, repeats)
    eng.set_timing(True)
    kern = []
    for it in range(2 + repeats):
        eng.load_weights_device(model)
        if it >= 2:
            kern.append(eng.weights_pack_ms())
    eng.set_timing(False)
    rec["pack_kernels_ms"] = spread(kern)
    nbytes = 4 * A * A + 2 * Np * Kp
    rec["bytes"] = nbytes
    rec["pack_gbs"] = nbytes / (rec["pack_kernels_ms"]["median"] * 1e-3) / 1e9
    rec["fraction_of_peak"] = rec["pack_gbs"] / PEAK_GBS
    rec["a_over_c"] = rec["a_host_ms"]["median"] / rec["c_inplace_ms"]["median"]
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weights_bench needs the GPU: there is nothing to measure without one")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "weights_bench.json"), "w") as f:
        for R in (14, 8):
            line = json.dumps(run(R, a.blocks, a.hidden, a.repeats))
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()


if __name__ == "__main__":
    main()
