#!/usr/bin/env python3
"""Device-resident replay (fpc_replay_*): what a training batch costs on the host path and on the device path.

    python3 tools/replay_bench.py --out DIR [--boards 14 8] [--batches 64 512 4096] [--records 8192]

Records come from a seeded generator (the start position's mailbox, a random side to move, 20-60 children with random
flat indices and visit counts) and are loaded with replay_load: no search runs.  Per board and batch size:
  host    wall time per batch of AlphaZero._batch's path: eng.encode([pod]) per sample + tuples.dense_pi per sample +
          stack + .to("cuda"), closed by a device synchronise;
  device  wall time per batch of DeviceReplayBuffer.sample (allocation of the three outputs, synchronise of torch's
          stream, slot upload, k_replay_decode, synchronise of the engine's stream);
  call    wall time of Engine.replay_batch alone into outputs made beforehand, and the HIP-event time of
          k_replay_decode alone in those same calls (fpc_set_timing): their difference is the slot upload, the launch
          and the closing stream synchronise;
  kernel  bytes written (24*R*R + A + 1 floats per sample) / event time, as a fraction of bench.PEAK_HBM_GBS.
Medians over the timed repeats (host: 2 warm-up + 7, device: 5 + 30) with min and max; DIR/replay_bench.json holds one JSON record per line (also printed)."""
import argparse
import json
import os
import random
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(HERE, "alphazero-4-player-chess_amd"), HERE]
import numpy as np
import torch

import fpc_ffi
import positions
import tuples
from bench import PEAK_HBM_GBS
from replay_buffer import DeviceReplayBuffer


def make_records(R, count, seed):
    A = (8 * R + 8) * R * R
    rng = np.random.default_rng(seed)
    turn, entries = positions.start_entries(R)
    start = fpc_ffi.board_from_dict(R, turn, entries)
    mailbox = np.frombuffer(bytes(start.sq), np.uint8, R * R).copy()
    recs = []
    for _ in range(count):
        n = int(rng.integers(20, 61))
        recs.append({"mailbox": mailbox, "turn": int(rng.integers(0, 4)), "z": float(rng.choice([-1.0, 1.0])),
                     "flat": np.sort(rng.choice(A, size=n, replace=False)).astype(np.int64),
                     "visits": rng.integers(1, 400, size=n).astype(np.int64)})
    return recs


def pod_of(rec):
    b = fpc_ffi.Board()
    C = fpc_ffi.C
    C.memmove(b.sq, rec["mailbox"].ctypes.data, rec["mailbox"].shape[0])
    b.turn = rec["turn"]
    for c in range(4):
        b.king[c] = fpc_ffi.NO_SQ
    return b


def spread(ms):
    a = np.asarray(ms, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max()), "repeats": int(a.size)}


def host_batch(eng, sample):
    """AlphaZero._batch, host replay"""
    x = np.concatenate([eng.encode([pod]) for pod, _ in sample])
    pi = torch.stack([tuples.dense_pi(rec, eng.A) for _, rec in sample])
    z = torch.tensor([rec["z"] for _, rec in sample], dtype=torch.float32).view(-1, 1)
    return torch.from_numpy(x).to("cuda"), pi.to("cuda"), z.to("cuda")


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def run(R, batches, count, seed):
    INV = {8: 2, 14: 3}[R]
    eng = fpc_ffi.Engine(R, INV, max_games=4, max_sims=4)
    recs = make_records(R, count, seed)
    host_items = [(pod_of(r), r) for r in recs]
    dbuf = DeviceReplayBuffer(eng, 0, count, rng=random.Random(seed), device="cuda")
    eng.replay_load(0, tuples.tuples_of(recs), count)
    hrng = random.Random(seed)
    out = []
    for bs in batches:
        rec = {"board": R, "batch": bs, "records": count, "bytes_written": bs * (24 * R * R + eng.A + 1) * 4}
        rec["host_ms"] = spread(timed(lambda: host_batch(eng, hrng.sample(host_items, bs)), 2, 7))
        rec["device_ms"] = spread(timed(lambda: dbuf.sample(bs), 5, 30))
        rec["host_over_device"] = rec["host_ms"]["median"] / rec["device_ms"]["median"]
        # the call alone and the kernel alone
        x = torch.empty((bs, 24, R, R), dtype=torch.float32, device="cuda")
        pi = torch.empty((bs, eng.A), dtype=torch.float32, device="cuda")
        z = torch.empty((bs,), dtype=torch.float32, device="cuda")
        slots = np.asarray(hrng.sample(range(count), bs), np.int32)
        eng.set_timing(True)
        call, kern = [], []
        for it in range(5 + 30):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.replay_batch(0, slots, x, pi, z)
            dt = 1e3 * (time.perf_counter() - t0)
            if it >= 5:
                call.append(dt)
                kern.append(eng.replay_decode_ms())
        eng.set_timing(False)
        rec["call_ms"], rec["kernel_ms"] = spread(call), spread(kern)
        rec["kernel_gbs"] = rec["bytes_written"] / (rec["kernel_ms"]["median"] * 1e-3) / 1e9
        rec["kernel_frac_hbm_peak"] = rec["kernel_gbs"] / PEAK_HBM_GBS
        rec["call_minus_kernel_ms"] = rec["call_ms"]["median"] - rec["kernel_ms"]["median"]
        out.append(rec)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--boards", type=int, nargs="+", default=[14, 8])
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 512, 4096])
    ap.add_argument("--records", type=int, default=8192)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("replay_bench needs the GPU: there is nothing to measure without one")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "replay_bench.json"), "w") as f:
        for R in a.boards:
            for rec in run(R, a.batches, a.records, seed=7):
                line = json.dumps(rec)
                print(line, flush=True)
                f.write(line + "\n")
                f.flush()


if __name__ == "__main__":
    main()
