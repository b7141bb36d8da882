"""Cases for the device-resident replay store (fpc_replay_*, k_replay_store, k_replay_decode), shared by the CPU tests
(wavefront-emulator build) and the GPU tests (product library).  The per-sample path that exists beside it --
Engine.encode of one board + tuples.dense_pi -- is the reference for every decoded row, bit for bit."""
import ctypes as C
import random

import numpy as np

import fpc_ffi
import tuples
from fpc_testlib import gold, make_engine, run_external_search
from net_cases import INV_OF, Spec, check_param_sums, load_extra
from replay_buffer import DeviceReplayBuffer, ReplayBuffer

EINVAL, ESTATE = -1, -9
TUPLE_BYTES = C.sizeof(fpc_ffi.Tuple)


def rec_of(board, R, flats, visits, z):
    return {"mailbox": np.frombuffer(bytes(board.sq), np.uint8, R * R).copy(), "turn": int(board.turn), "z": float(z),
            "flat": np.asarray(flats, np.int64), "visits": np.asarray(visits, np.int64)}


def board_of_rec(rec):
    """the board tuples.dense_batch encodes for a record"""
    b = fpc_ffi.Board()
    for i, v in enumerate(rec["mailbox"]):
        b.sq[i] = int(v)
    b.turn = rec["turn"]
    for c in range(4):
        b.king[c] = fpc_ffi.NO_SQ
    return b


def decode(eng, backend, ring, slots):
    """replay_batch into NaN-filled outputs (an element the kernel leaves out shows), back as numpy"""
    n, R, A = len(slots), eng.R, eng.A
    if backend == "emul":
        enc, pi, z = (np.full(s, np.nan, np.float32) for s in ((n, 24, R, R), (n, A), (n,)))
        eng.replay_batch(ring, slots, enc, pi, z)
        return enc, pi, z
    import torch
    enc, pi, z = (torch.full(s, float("nan"), dtype=torch.float32, device="cuda") for s in ((n, 24, R, R), (n, A), (n,)))
    torch.cuda.synchronize()
    eng.replay_batch(ring, slots, enc, pi, z)
    return enc.cpu().numpy(), pi.cpu().numpy(), z.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def expected_rows(eng, recs):
    """per record: (Engine.encode of its board alone, dense_pi -- zeros for n == 0, z as f32), computed once"""
    out = []
    for r in recs:
        pi = tuples.dense_pi(r, eng.A).numpy() if len(r["flat"]) else np.zeros(eng.A, np.float32)
        out.append((eng.encode([board_of_rec(r)])[0], pi, np.float32(r["z"])))
    return out


# ---- 1. the reference's recorded training batch ----------------------------------------------------
def case_golden(backend):
    import torch
    import torch.nn.functional as F
    import net
    R = 8
    x = load_extra(R)["train_batch"]
    eng = make_engine(backend, R, INV_OF[R], max_games=4, max_sims=4)
    recs = []
    for t in x["tuples"]:
        b = fpc_ffi.board_from_lists(R, t["state"]["turn"], t["state"]["pl"])
        recs.append(rec_of(b, R, [c[0] for c in t["pi"]], [c[1] for c in t["pi"]], t["z"]))
    n = len(recs)
    assert n == 16
    eng.replay_reserve(0, n)
    eng.replay_load(0, tuples.tuples_of(recs), n)
    enc, pi, z = decode(eng, backend, 0, list(range(n)))
    eng.close()
    for i, (t, r) in enumerate(zip(x["tuples"], recs)):
        nz = np.nonzero(enc[i].reshape(-1))[0]
        assert nz.tolist() == t["enc"], i
        assert np.all(enc[i].reshape(-1)[nz] == 1.0)
        assert np.array_equal(bits(pi[i]), bits(tuples.dense_pi(r, eng.A).numpy())), i
        assert bits(z[i:i + 1])[0] == bits(np.float32(t["z"]).reshape(1))[0], i
    torch.manual_seed(x["seed"])
    model = net.ResNet(Spec(R), x["blocks"], x["hidden"], "cpu")
    check_param_sums(model, x["pnames"], x["psums"])
    et, pt, zt = torch.from_numpy(enc), torch.from_numpy(pi), torch.from_numpy(z).view(-1, 1)
    for mode in ("train", "eval"):
        model.train(mode == "train")
        with torch.no_grad():
            out_policy, out_value = model(et)
            pl = float(F.cross_entropy(out_policy, pt))
            vl = float(F.mse_loss(out_value.squeeze(), zt.squeeze()))
        ref = x["losses"][mode]
        assert abs(pl - ref[0]) < 2e-5 * abs(ref[0]) and abs(vl - ref[1]) < 2e-5 * max(abs(ref[1]), 1e-3), (mode, pl, vl, ref)
    return n


# ---- 2. against the per-sample path, bit for bit ---------------------------------------------------
def edge_records(R, seed=5):
    """positions of the golden playouts (consecutive plies: all four sides to move, so all four rotations) with hand-made
    sparse policies: n = 0, 1, 64, 65, 256 (the lane-loop edges and FPC_TUPLE_MAXC) and a few of 20..60, flat indices 0
    and A-1, visit counts 1 and 65535"""
    A = (8 * R + 8) * R * R
    rng = np.random.default_rng(seed)
    snaps = [s["before"] for p in gold(R)["playouts"][:2] for s in p[:6]]
    recs = []
    for k, n in enumerate([0, 1, 64, 65, 256, 20, 37, 60, 2, 41, 256, 33]):
        snap = snaps[k % len(snaps)]
        b = fpc_ffi.board_from_lists(R, snap["turn"], snap["pl"])
        flats = rng.choice(A, size=n, replace=False)
        visits = rng.integers(1, 65536, size=n)
        if n >= 2:
            flats[0], flats[-1] = 0, A - 1
            flats = np.unique(flats)
            visits = visits[:len(flats)]
            visits[0], visits[-1] = 1, 65535
        elif n == 1:
            flats[0], visits[0] = (A - 1, 65535) if k % 2 else (0, 1)
        recs.append(rec_of(b, R, flats, visits, (-1.0, 0.34, 1.0)[k % 3]))
    assert {r["turn"] for r in recs} == {0, 1, 2, 3} and max(len(r["flat"]) for r in recs) == 256
    return recs


def case_matches_per_sample_path(backend, R, rules):
    eng = make_engine(backend, R, INV_OF[R], max_games=4, max_sims=4)
    eng.set_rules(rules)
    recs = edge_records(R)
    nrec = len(recs)
    want = expected_rows(eng, recs)
    eng.replay_reserve(1, nrec + 3)
    eng.replay_load(1, tuples.tuples_of(recs), nrec)
    done = 0
    for slots in ([4], [7, 7, 0], [(200 - 3 * i) % nrec for i in range(67)], list(range(nrec - 1, -1, -1))):
        enc, pi, z = decode(eng, backend, 1, slots)
        for i, s in enumerate(slots):
            assert np.array_equal(bits(enc[i]), bits(want[s][0])), (slots, i)
            assert np.array_equal(bits(pi[i]), bits(want[s][1])), (slots, i)
            assert bits(z[i:i + 1])[0] == bits(want[s][2].reshape(1))[0], (slots, i)
            done += 1
    eng.close()
    return done


# ---- 3. ring semantics against replay_buffer.ReplayBuffer ------------------------------------------
def _ring_bytes(eng, ring):
    arr, n = eng.replay_read(ring)
    raw = bytes(memoryview(arr).cast("B"))
    return [raw[i * TUPLE_BYTES:(i + 1) * TUPLE_BYTES] for i in range(n)]


PUSHES = [([4, 0, 2], [0, 0, 0]),
          ([5, 1, 3, 0], [0, 0, -1, 0]),                       # ring 0 wraps
          ([2, 2, 5, 4, 0, 1, 3], [0, 0, 0, 0, 0, 0, 1]),      # more than the capacity in one call
          ([3, 1, 0, 5, 4, 2, 2], [1, -1, 1, 1, 1, 1, 1])]


def case_ring_semantics(backend, gathered=False):
    import evaluators
    import positions
    R, G, sims, CAP = 8, 3, 6, 5
    eng = make_engine(backend, R, INV_OF[R], max_games=G, max_sims=sims)
    turn, entries = positions.start_entries(R)
    boards = [fpc_ffi.board_from_dict(R, turn, entries) for _ in range(G)]
    ev = evaluators.make("hash", R)
    eng.tuples_reserve(2 * G)
    for ply in range(2):
        res = run_external_search(eng, backend, boards, sims, 3.0, ev)
        eng.collect_tuples([7, 3, 5], ply)
        boards = eng.take_action(boards, [int(res["flat"][g, ply]) for g in range(G)])
    eng.tuples_set_z([3, 5, 7], [1.0, -1.0, 0.25], [-1.0, 1.0, -0.25])
    arr, n = eng.tuples_read()
    assert n == 2 * G
    raw = bytes(memoryview(arr).cast("B"))
    src = [raw[i * TUPLE_BYTES:(i + 1) * TUPLE_BYTES] for i in range(n)]
    assert len(set(src)) == n
    sources = [fpc_ffi.REPLAY_COLLECTED]
    if gathered:
        eng.comm_init(fpc_ffi.comm_unique_id(), 0, 1)
        counts, total = eng.allgather_tuples_device()
        assert total == n and counts[0] == n
        sources.append(fpc_ffi.REPLAY_GATHERED)
    for source in sources:
        eng.replay_reserve(0, CAP)                      # also empties a ring that was in use
        eng.replay_reserve(1, CAP)
        host = [ReplayBuffer(CAP), ReplayBuffer(CAP)]
        assert eng.replay_size(0) == 0 and eng.replay_size(1) == 0
        for idx, ring_of in PUSHES:
            eng.replay_push(source, idx, ring_of)
            for i, r in zip(idx, ring_of):
                if r >= 0:
                    host[r].add(src[i])
            for r in (0, 1):
                assert eng.replay_size(r) == len(host[r])
                assert _ring_bytes(eng, r) == host[r]._items, (source, idx, r)
        eng.replay_reserve(0, CAP)                      # src_index None: 0..m-1; ring_of None: everything to ring 0
        eng.replay_push(source, None, None, 4)
        assert _ring_bytes(eng, 0) == src[:4]
    eng.close()
    return len(sources)


# ---- 4. errors ---------------------------------------------------------------------------------------
def case_errors(backend):
    R = 8
    eng = make_engine(backend, R, INV_OF[R], max_games=2, max_sims=4)
    L, h, P = eng.L, eng.h, C.POINTER
    recs = edge_records(R)[:4]
    arr = tuples.tuples_of(recs)

    def failed(rc, want):
        assert rc == want, (rc, want)
        assert (L.fpc_last_error(h) or b"").decode() != ""
        return True

    i4 = (C.c_int * 4)(0, 1, 2, 3)
    r4 = (C.c_int8 * 4)(0, 0, 0, 0)
    out = np.zeros(4 * eng.A, np.float32)
    ptr = out.ctypes.data
    # nothing reserved yet
    assert failed(L.fpc_replay_load(h, 0, arr, 4), ESTATE)
    assert failed(L.fpc_replay_batch(h, 0, i4, 1, ptr, ptr, ptr), ESTATE)
    assert failed(L.fpc_replay_reserve(h, 3, 5), EINVAL) and failed(L.fpc_replay_reserve(h, -1, 5), EINVAL)
    assert failed(L.fpc_replay_reserve(h, 0, 0), EINVAL)
    assert L.fpc_replay_size(h, 3) == EINVAL and L.fpc_replay_size(h, 1) == 0
    eng.replay_reserve(0, 6)
    eng.replay_load(0, arr, 4)
    eng.tuples_reserve(4)                                  # no collected tuples: every source index is out of range
    before = _ring_bytes(eng, 0)
    assert failed(L.fpc_replay_push(h, fpc_ffi.REPLAY_COLLECTED, i4, r4, 1), EINVAL)
    assert failed(L.fpc_replay_push(h, fpc_ffi.REPLAY_GATHERED, i4, r4, 1), ESTATE)
    assert failed(L.fpc_replay_push(h, 2, i4, r4, 1), EINVAL) and failed(L.fpc_replay_push(h, 0, i4, r4, -1), EINVAL)
    assert failed(L.fpc_replay_load(h, 3, arr, 1), EINVAL) and failed(L.fpc_replay_load(h, 0, arr, -1), EINVAL)
    assert failed(L.fpc_replay_load(h, 1, arr, 1), ESTATE)
    assert failed(L.fpc_replay_batch(h, 3, i4, 1, ptr, ptr, ptr), EINVAL) and failed(L.fpc_replay_batch(h, 0, i4, -1, ptr, ptr, ptr), EINVAL)
    for nul in range(3):
        a = [ptr, ptr, ptr]
        a[nul] = None
        assert failed(L.fpc_replay_batch(h, 0, i4, 1, *a), EINVAL)
    assert failed(L.fpc_replay_batch(h, 0, (C.c_int * 2)(0, 4), 2, ptr, ptr, ptr), EINVAL)     # size is 4
    assert failed(L.fpc_replay_batch(h, 0, (C.c_int * 2)(-1, 0), 2, ptr, ptr, ptr), EINVAL)
    assert failed(L.fpc_replay_batch(h, 1, i4, 1, ptr, ptr, ptr), ESTATE)
    one = (fpc_ffi.Tuple * 1)()
    assert failed(L.fpc_replay_read(h, 0, one, 4, 1), EINVAL) and failed(L.fpc_replay_read(h, 3, one, 0, 1), EINVAL)
    assert eng.replay_size(0) == 4 and _ring_bytes(eng, 0) == before
    eng.close()
    # source indices and ring_of values against collected tuples that do exist
    import evaluators
    import positions
    eng = make_engine(backend, R, INV_OF[R], max_games=2, max_sims=4)
    L, h = eng.L, eng.h
    turn, entries = positions.start_entries(R)
    boards = [fpc_ffi.board_from_dict(R, turn, entries) for _ in range(2)]
    eng.tuples_reserve(2)
    run_external_search(eng, backend, boards, 4, 3.0, evaluators.make("hash", R))
    eng.collect_tuples(None, 0)
    eng.replay_reserve(0, 3)
    eng.replay_push(fpc_ffi.REPLAY_COLLECTED, [1], [0])
    before = _ring_bytes(eng, 0)
    assert failed(L.fpc_replay_push(h, 0, (C.c_int * 2)(0, 2), (C.c_int8 * 2)(0, 0), 2), EINVAL)     # two collected tuples
    assert failed(L.fpc_replay_push(h, 0, (C.c_int * 2)(0, -1), (C.c_int8 * 2)(0, 0), 2), EINVAL)
    assert failed(L.fpc_replay_push(h, 0, None, None, 3), EINVAL)
    assert failed(L.fpc_replay_push(h, 0, (C.c_int * 2)(0, 1), (C.c_int8 * 2)(0, 2), 2), EINVAL)
    assert failed(L.fpc_replay_push(h, 0, (C.c_int * 2)(0, 1), (C.c_int8 * 2)(0, -2), 2), EINVAL)
    assert failed(L.fpc_replay_push(h, 0, (C.c_int * 2)(0, 1), (C.c_int8 * 2)(0, 1), 2), ESTATE)     # ring 1 never reserved
    assert eng.replay_size(0) == 1 and _ring_bytes(eng, 0) == before
    eng.close()
    return True


# ---- 5. DeviceReplayBuffer.sample -------------------------------------------------------------------
def case_device_buffer_sample(backend):
    R = 8
    eng = make_engine(backend, R, INV_OF[R], max_games=2, max_sims=4)
    recs = edge_records(R)
    recs = [r for r in recs if len(r["flat"])]
    want = expected_rows(eng, recs)
    dbuf = DeviceReplayBuffer(eng, 0, 9, rng=random.Random(3), device=None if backend == "emul" else "cuda")
    hbuf = ReplayBuffer(9, rng=random.Random(3))
    eng.replay_load(0, tuples.tuples_of(recs), len(recs))          # 11 records into 9 slots: the ring has wrapped
    for i in range(len(recs)):
        hbuf.add(i)
    assert len(dbuf) == len(hbuf) == 9
    for bs in (4, 9):
        x, pi, z = dbuf.sample(bs)
        picked = hbuf.sample(bs)
        assert tuple(x.shape) == (bs, 24, R, R) and tuple(pi.shape) == (bs, eng.A) and tuple(z.shape) == (bs, 1)
        assert (x.is_cuda and pi.is_cuda and z.is_cuda) == (backend != "emul")
        x, pi, z = x.cpu().numpy(), pi.cpu().numpy(), z.cpu().numpy()
        for i, s in enumerate(picked):
            assert np.array_equal(bits(x[i]), bits(want[s][0])) and np.array_equal(bits(pi[i]), bits(want[s][1]))
            assert bits(z[i])[0] == bits(want[s][2].reshape(1))[0]
    # tuples.dense_batch_device: the three tensors of dense_batch
    e2, p2, z2 = tuples.dense_batch_device(eng, recs, device=None if backend == "emul" else "cuda")
    e1, p1, z1 = tuples.dense_batch(eng, recs)
    assert np.array_equal(bits(e2.cpu().numpy()), bits(e1.numpy())) and np.array_equal(bits(p2.cpu().numpy()), bits(p1.numpy()))
    assert np.array_equal(bits(z2.cpu().numpy()), bits(z1.numpy())) and tuple(z2.shape) == (len(recs), 1)
    # the scratch ring only grows: a smaller batch afterwards decodes the same rows out of the allocation that is there
    e3, p3, z3 = tuples.dense_batch_device(eng, recs[:3], device=None if backend == "emul" else "cuda")
    assert eng.replay_cap[fpc_ffi.REPLAY_SCRATCH] == len(recs) and eng.replay_size(fpc_ffi.REPLAY_SCRATCH) == 3
    assert np.array_equal(bits(e3.cpu().numpy()), bits(e1.numpy()[:3])) and np.array_equal(bits(p3.cpu().numpy()), bits(p1.numpy()[:3]))
    # outputs that do not start on a 16-byte boundary are refused with a message, not written
    import torch
    odd = torch.empty(4 * eng.A + 1, dtype=torch.float32, device=x2dev(backend))[1:]
    xs, zs = torch.empty((4, 24, R, R), dtype=torch.float32, device=x2dev(backend)), torch.empty(4, dtype=torch.float32, device=x2dev(backend))
    try:
        eng.replay_batch(0, [0, 1, 2, 3], xs, odd, zs)
        raise AssertionError("an unaligned pi was accepted")
    except ValueError as ex:
        assert "16-byte" in str(ex)
    # one ring per engine and number: a second buffer on it empties it, and the first one says so instead of decoding
    other = DeviceReplayBuffer(eng, 0, 9, device=dbuf.device)
    assert len(other) == 0
    for use in (lambda: len(dbuf), lambda: dbuf.sample(1)):
        try:
            use()
            raise AssertionError("a buffer whose ring was reserved again went on")
        except RuntimeError as ex:
            assert "reserved again" in str(ex)
    eng.close()
    return True


def x2dev(backend):
    return "cpu" if backend == "emul" else "cuda"


# ---- 6. AlphaZero with args["device_replay"] ---------------------------------------------------------
def case_alphazero_equivalence(backend, reuse):
    import torch

    import dropin_cases
    R = 8
    dropin_cases.setup(backend, R)
    import alphazero_cpp as az
    from alphazero import AlphaZero
    from fen_parser import parse_board_args_from_fen
    from four_player_chess_board import FourPlayerChess
    args = {"C": 3.0, "num_searches": 8, "num_parallel_games": 3, "temperature": 1.0, "heuristic_weight": 0.02,
            "max_game_length": 6, "replay_buffer_capacity": 40, "validation_buffer_capacity": 10, "reuse_tree": reuse}
    init = parse_board_args_from_fen(FourPlayerChess.start_fen, R)
    model = torch.nn.Linear(1, 1)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    made = {}
    for dev in (False, True):
        a = AlphaZero(model, opt, FourPlayerChess, dict(args, device_replay=dev), init, evaluator=dropin_cases.Eval("hash", R), seed=11)
        a.play()
        a.play()                                        # the second episode appends to what the first left
        made[dev] = a
    host, devc = made[False], made[True]
    eng = az.engine()
    assert len(host.experience_buffer) + len(host.validation_buffer) == 36
    for ring, (hb, db) in enumerate(((host.experience_buffer, devc.experience_buffer), (host.validation_buffer, devc.validation_buffer))):
        assert len(db) == len(hb) == eng.replay_size(ring) and len(hb) > 0
        arr, n = eng.replay_read(ring)
        for r, (pod, flats, visits, z) in zip(tuples.records_of(arr, n, R), hb._items):
            assert r["mailbox"].tobytes() == bytes(pod.sq)[:R * R] and r["turn"] == pod.turn
            assert r["flat"].tolist() == list(flats) and r["visits"].tolist() == list(visits)
            assert np.float32(r["z"]) == np.float32(z)
    bs = 5
    host.experience_buffer._rng = random.Random(9)
    devc.experience_buffer._rng = random.Random(9)
    xh, ph, zh = host._batch(host.experience_buffer.sample(bs))
    xd, pd, zd = devc._batch(devc.experience_buffer.sample(bs))
    for u, v in ((xh, xd), (ph, pd), (zh, zd)):
        assert u.shape == v.shape and np.array_equal(bits(u.cpu().numpy()), bits(v.cpu().numpy()))
    return True
