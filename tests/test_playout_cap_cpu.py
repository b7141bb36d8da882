"""Playout cap randomization without a GPU: the cap on the inputs of the engine cases (tests/playout_cap_cases.py) from the
model alone, mcts.budgets_for with fast rows, the ValueErrors, selfplay.play's draw of fast and full plies, and
alphazero.AlphaZero with args["playout_cap"] on the wavefront-emulator engine -- buffer contents, host and device replay
batches, the weighted policy loss by hand, and a seeded run WITHOUT the key against the episodes the parent commit recorded
(tests/golden/playout_cap_parent_episodes.json).  Everything is compared exactly."""
import json
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import evaluators
import forced_cases as fc
import fpc_ffi
import mcts
import playout_cap_cases as pc
import search_model as sm
import selfplay
from fpc_testlib import make_engine, roots_of

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "playout_cap_parent_episodes.json")


def test_conditions_of_the_engine_cases():
    """every case: a full row where forcing decided a selection and pruning took a visit out, and a fast row whose tree would
    differ if forced; the play case has a root proven WIN or DRAW"""
    assert pc.conditions() == len(pc.CASES)
    assert pc.proven_root_case() in pc.CASES


def test_model_without_a_mask_is_the_forced_model():
    case = pc.CASES[1]
    assert case in fc.CASES
    _, _, forced = fc.searched_model(case)
    mine = pc.all_full_model(case)
    assert [pc._kids(mine, g) for g in range(case[5])] == [pc._kids(forced, g) for g in range(case[5])]
    assert mine.targets() == forced.targets() and mine.sims_done == forced.sims_done


# ---- budgets_for ------------------------------------------------------------------------------------------------------------
def test_budgets_for_with_fast_rows():
    kept = [1, 5, 1, 30]
    assert mcts.budgets_for(kept, 16, 32, "per_game") == [16, 16, 16, 3]                  # as it was
    assert mcts.budgets_for(kept, 16, 32, "per_game", fast=[0, 1, 1, 0], fast_searches=4) == [16, 4, 4, 3]
    assert mcts.budgets_for(kept, 16, 32, "per_game", fast=[0, 0, 0, 1], fast_searches=4) == [16, 16, 16, 3]   # the handle's room still caps
    assert mcts.budgets_for(kept, 16, 32, "visit_target", fast=[1, 1, 0, 0], fast_searches=4) == [4, 0, 16, 0]
    assert mcts.budgets_for([0, 4, 0], 16, 32, "per_game", born=0, fast=[True, True, False], fast_searches=4) == [4, 4, 16]
    assert mcts.budgets_for(kept, 16, 32, None, fast=[0, 1, 1, 0], fast_searches=4) is None
    assert mcts.budgets_for(kept, 16, 32, "per_game", fast=None, fast_searches=4) == [16, 16, 16, 3]
    with pytest.raises(ValueError):
        mcts.budgets_for(kept, 16, 32, "per_game", fast=[0, 1], fast_searches=4)
    with pytest.raises(ValueError):
        mcts.budgets_for(kept, 16, 32, "per_game", fast=[0, 1, 1, 0])


@pytest.mark.parametrize("cap", [{"full_prob": 0.0, "fast_searches": 2}, {"full_prob": -0.5, "fast_searches": 2},
                                 {"full_prob": 1.5, "fast_searches": 2}, {"full_prob": float("nan"), "fast_searches": 2},
                                 {"full_prob": 0.5, "fast_searches": 0}, {"full_prob": 0.5, "fast_searches": 9},
                                 {"full_prob": 0.5, "fast_searches": 2.5}, {"full_prob": "0.5", "fast_searches": 2},
                                 {"full_prob": 0.5}, {"fast_searches": 2}, 0.25, [0.25, 2], True],
                         ids=lambda c: str(c))
def test_bad_playout_cap_raises(cap):
    args = {"C": 3.0, "num_searches": 8, "playout_cap": cap}
    with pytest.raises(ValueError):
        mcts.MCTS(None, lambda x: x, args)
    with pytest.raises(ValueError):
        mcts.parse_playout_cap(cap, 8)


def test_good_playout_cap_and_fast_without_it():
    assert mcts.parse_playout_cap(None, 8) is None
    assert mcts.parse_playout_cap({"full_prob": 1, "fast_searches": 8, "record_fast": True}, 8) == (1.0, 8)
    assert mcts.parse_playout_cap({"full_prob": 0.25, "fast_searches": 1}, 8) == (0.25, 1)
    m = mcts.MCTS(None, lambda x: x, {"C": 3.0, "num_searches": 8})
    assert m.playout_cap is None
    with pytest.raises(ValueError):
        m.search([], fast=[])                        # fast= needs args["playout_cap"]
    m = mcts.MCTS(None, lambda x: x, {"C": 3.0, "num_searches": 8, "playout_cap": {"full_prob": 0.5, "fast_searches": 2}})
    assert m.playout_cap == (0.5, 2)
    with pytest.raises(ValueError):
        m._fast_rows([True], 2)
    assert m._fast_budgets([0, 0, 3], [1, 0, 1], 16) == [2, 8, 2]      # sim_budget None counts as "per_game"


def test_wire_records_carry_the_fast_flag():
    """tuples.pack_record / unpack_records: bit 7 of the turn byte is the flag, the turn its low bits; without the flag the
    bytes are what they were"""
    import tuples
    Rr = 8
    mailbox = bytes(range(Rr * Rr))
    recs = [(3, -1.0, [5, 4607], [1, 65535], True), (0, 0.5, [], [], True), (2, 1.0, [7], [9], False)]
    blob = b"".join(tuples.pack_record(Rr, mailbox, t, z, f, v, fast=fa) for t, z, f, v, fa in recs)
    plain = b"".join(tuples.pack_record(Rr, mailbox, t, z, f, v) for t, z, f, v, _ in recs)
    assert len(blob) == len(plain) and tuples.pack_record(Rr, mailbox, 2, 1.0, [7], [9], fast=False) == tuples.pack_record(Rr, mailbox, 2, 1.0, [7], [9])
    assert [i for i in range(len(blob)) if blob[i] != plain[i]] == [Rr * Rr, 2 * Rr * Rr + 7 + 8]      # the two flagged turn bytes
    assert blob[Rr * Rr] == 0x83 and plain[Rr * Rr] == 3
    out = tuples.unpack_records(Rr, blob)
    assert [(r["turn"], r["z"], r["flat"].tolist(), r["visits"].tolist(), r["fast"]) for r in out] == [(t, z, f, v, fa) for t, z, f, v, fa in recs]
    assert [r["fast"] for r in tuples.unpack_records(Rr, plain)] == [False] * 3
    assert all(bytes(r["mailbox"]) == mailbox for r in out)
    back = tuples.records_of(tuples.tuples_of(out), 3, Rr)                               # and through the fixed-size record
    assert [r["fast"] for r in back] == [True, True, False] and [r["turn"] for r in back] == [3, 0, 2]
    assert tuples.weights_of(out).view(-1).tolist() == [0.0, 0.0, 1.0]


def test_the_models_gated_search_row_by_row():
    """the model's own search under a mixed mask, against the models it was copied from: every rule set used holds
    FPC_RULES_ROTATION, so a full row is the row of forced_model.Model's search of the same inputs and a fast row the row of
    the same search with factor 0 (solver_model.Model's loop), trees, targets and proofs"""
    import forced_model as fm
    for case in pc.CASES:
        pos, rules, fpu, solver, K, G, sims, seed = case
        assert rules & 4
        _, _, mask, mixed = pc.searched_model(case)
        boards, gamma = fc.boards_for(pos, rules, G), fc.gamma_for(G, seed)
        full = fc._model(fm.Model, boards, rules, fpu, solver, gamma, forced=pc.FACTOR)
        plain = fc._model(fm.Model, boards, rules, fpu, solver, gamma, forced=0.0)
        assert full.search(sims, K) == 0 and plain.search(sims, K) == 0
        for g in range(G):
            ref = plain if mask[g] else full
            assert pc._kids(mixed, g) == pc._kids(ref, g) and mixed.roots[g].N == ref.roots[g].N, (case, g)
            assert mixed.targets()[g] == ref.targets()[g] and mixed.sims_done[g] == ref.sims_done[g], (case, g)
            assert mixed.proofs()[0][g] == ref.proofs()[0][g] and list(mixed.proofs()[1][g]) == list(ref.proofs()[1][g]), (case, g)


# ---- selfplay.play ------------------------------------------------------------------------------------------------------------
def _loop(cap, cap_uniforms, refill):
    R, INV, G, sims, L = 8, 2, 3, 6, 4
    import positions
    turn, entries = positions.start_entries(R)
    from oracle import orc
    n_games = G + (2 if refill else 0)
    boards = roots_of([orc.board_from_dict(R, turn, [list(e) for e in entries]) for _ in range(n_games)], R)
    ev = evaluators.make("hash", R)
    args = {"temperature": 1.0, "max_game_length": L, "heuristic_weight": 0.5}
    uniforms = np.random.default_rng(5).random((L, n_games)).tolist()
    eng = make_engine("emul", R, INV, max_games=G, max_sims=sims)
    calls = []

    def plain_search(pods):                          # a one-argument caller, as every caller was
        calls.append(None)
        eng.search_begin(pods, 3.0)
        sm.run_steps(eng, "emul", sims, ev)
        return eng.search_results(roots=pods)

    def capped_search(pods, fast=None):
        calls.append(list(fast))
        eng.search_begin(pods, 3.0)
        sm.run_steps(eng, "emul", sims, ev)
        return eng.search_results(roots=pods)

    try:
        eng.set_rules(15)
        if cap is None:
            eps = selfplay.play(plain_search, eng, boards[:G], args, uniforms, refill=boards[G:] or None)
        else:
            eps = selfplay.play(capped_search, eng, boards[:G], args, uniforms, refill=boards[G:] or None, playout_cap=cap,
                                cap_uniforms=cap_uniforms)
    finally:
        eng.set_rules(0)
        eng.close()
    return eps, calls


@pytest.mark.parametrize("refill", [False, True], ids=["plain", "refill"])
def test_play_draws_fast_and_full_plies(refill):
    L, n_games = 4, 5 if refill else 3
    cu = np.random.default_rng(77).random((L, n_games)).tolist()
    cap = {"full_prob": 0.5, "fast_searches": 2}
    eps, calls = _loop(cap, cu, refill)
    base, base_calls = _loop(None, None, refill)
    assert all(c is None for c in base_calls) and all(isinstance(c, list) for c in calls) and len(calls) == len(base_calls)
    seen = set()
    for e, b in zip(eps, base):
        assert len(e.fast) == len(e.entries) == e.length and all(len(x) == 3 for x in e.entries)
        assert e.fast == [cu[p][e.gid] >= 0.5 for p in range(e.length)]                  # the game's OWN ply
        assert b.fast == [False] * b.length
        assert e.moves == b.moves and e.z == b.z        # this scripted search ignores the flag: the games are the same
        seen.update(e.fast)
    assert seen == {True, False}
    # the lists handed to search_fn are the batch's, in batch order: step 0 is games 0..G-1 at ply 0
    assert calls[0] == [cu[0][g] >= 0.5 for g in range(3)]
    assert sum(len(c) for c in calls) == sum(e.length for e in eps)
    if refill:
        assert any(e.start > 0 for e in eps)
    # full_prob = 1: nothing is fast, whatever the draws
    eps, calls = _loop({"full_prob": 1.0, "fast_searches": 2}, cu, refill)
    assert not any(any(e.fast) for e in eps) and not any(any(c) for c in calls)


def test_play_refuses_a_bad_cap():
    with pytest.raises(ValueError):
        selfplay.play(None, None, [], {"temperature": 1.0, "max_game_length": 1, "heuristic_weight": 0.5}, [],
                      playout_cap={"full_prob": 0.0, "fast_searches": 1}, cap_uniforms=[[]])
    with pytest.raises(ValueError):
        selfplay.play(None, None, [], {"temperature": 1.0, "max_game_length": 1, "heuristic_weight": 0.5}, [],
                      playout_cap={"full_prob": 0.5, "fast_searches": 1})
    with pytest.raises(ValueError):                                                      # cap_uniforms of the wrong shape
        selfplay.play(None, None, [None, None], {"temperature": 1.0, "max_game_length": 2, "heuristic_weight": 0.5}, [],
                      playout_cap={"full_prob": 0.5, "fast_searches": 1}, cap_uniforms=[[0.1, 0.2]])
    with pytest.raises(ValueError):
        selfplay.play(None, None, [None, None], {"temperature": 1.0, "max_game_length": 1, "heuristic_weight": 0.5}, [], refill=[None],
                      playout_cap={"full_prob": 0.5, "fast_searches": 1}, cap_uniforms=[[0.1, 0.2]])


# ---- alphazero.AlphaZero on the emulator engine ---------------------------------------------------------------------------
R = 8
ARGS = {"C": 3.0, "num_searches": 8, "num_parallel_games": 3, "temperature": 1.0, "heuristic_weight": 0.02,
        "max_game_length": 6, "replay_buffer_capacity": 60, "validation_buffer_capacity": 20, "reuse_tree": True,
        "rules": "selfplay", "fpu": 0.25, "root_noise": True, "dirichlet_alpha": 0.3, "dirichlet_epsilon": 0.25, "noise_seed": 3,
        "forced_playouts": 2.0, "sim_budget": "per_game", "live_rows": True, "batch_size": 4}
CAP = {"full_prob": 0.5, "fast_searches": 2}


class Tiny(torch.nn.Module):
    """a policy / value pair that depends on the input, cheap enough for a CPU test"""
    def __init__(self, A):
        super().__init__()
        self.a = torch.nn.Parameter(torch.tensor(0.125))
        self.ramp = torch.linspace(-1.0, 1.0, A)

    def forward(self, x):
        h = (x.flatten(1) * torch.arange(x[0].numel(), dtype=torch.float32).remainder(7.0)).sum(1, keepdim=True) * self.a
        return h * self.ramp, torch.tanh(h * 0.0625)


def _alphazero(extra, device_replay, total_games=None, plays=2, seed=11):
    import dropin_cases
    dropin_cases.setup("emul", R)
    from alphazero import AlphaZero
    from fen_parser import parse_board_args_from_fen
    from four_player_chess_board import FourPlayerChess
    init = parse_board_args_from_fen(FourPlayerChess.start_fen, R)
    model = Tiny(FourPlayerChess.action_space_size)
    opt = torch.optim.SGD(model.parameters(), lr=0.1)
    a = AlphaZero(model, opt, FourPlayerChess, dict(ARGS, device_replay=device_replay, **extra), init,
                  evaluator=dropin_cases.Eval("hash", R), seed=seed)
    episodes = [a.play(total_games) for _ in range(plays)]
    return a, episodes


def _episode_dump(episodes):
    return [[{"gid": e.gid, "start": e.start, "moves": [int(m) for m in e.moves], "z": [float(z) for z in e.z], "result": int(e.result),
              "entries": [[int(b.turn), [int(f) for f in fl], [int(v) for v in vi]] for b, fl, vi in e.entries]} for e in eps]
            for eps in episodes]


def _ring_records(a, ring):
    import alphazero_cpp as az
    import tuples
    arr, n = az.engine().replay_read(ring)
    return tuples.records_of(arr, n, R)


def test_without_the_key_a_seeded_run_is_the_parent_commits():
    """args without "playout_cap": the episodes and buffers of a seeded run are those the parent commit produced (no extra
    draw from the generator, no new call)"""
    want = json.load(open(GOLDEN))
    for key, device_replay in (("host", False), ("device", True)):
        a, episodes = _alphazero({}, device_replay)
        assert a.playout_cap is None and not a.record_fast
        assert _episode_dump(episodes) == want["episodes"], key
        assert [len(a.experience_buffer), len(a.validation_buffer)] == want["buffers"], key
        assert all(not any(e.fast) for eps in episodes for e in eps)
        if device_replay:
            assert not any(r["fast"] for ring in (0, 1) for r in _ring_records(a, ring))


def _stored(a, ring, device_replay):
    """the buffer's records as (mailbox bytes, turn, flats, visits, f32 z, fast) in slot order"""
    if device_replay:
        return [(r["mailbox"].tobytes(), r["turn"], r["flat"].tolist(), r["visits"].tolist(), np.float32(r["z"]), r["fast"])
                for r in _ring_records(a, ring)]
    buf = a.experience_buffer if ring == 0 else a.validation_buffer
    return [(bytes(it[0].sq)[:R * R], int(it[0].turn), [int(f) for f in it[1]], [int(v) for v in it[2]], np.float32(it[3]),
             (it[4] == 0.0) if len(it) > 4 else False) for it in buf._items]


@pytest.mark.parametrize("record_fast", [False, True], ids=["drop_fast", "record_fast"])
def test_alphazero_with_the_cap(record_fast):
    cap = dict(CAP, record_fast=record_fast)
    host, eps_h = _alphazero({"playout_cap": cap}, False)
    stored_h = [_stored(host, ring, False) for ring in (0, 1)]
    dev, eps_d = _alphazero({"playout_cap": cap}, True)
    stored_d = [_stored(dev, ring, True) for ring in (0, 1)]
    assert _episode_dump(eps_h) == _episode_dump(eps_d)
    fast_flags = [f for eps in eps_h for e in eps for f in e.fast]
    assert [f for eps in eps_d for e in eps for f in e.fast] == fast_flags and {True, False} == set(fast_flags)
    n_full, n_all = fast_flags.count(False), len(fast_flags)
    # buffer contents: the same records in the same slots on both paths; fast plies are left out, or flagged
    assert stored_h == stored_d
    everything = stored_h[0] + stored_h[1]
    assert len(everything) == (n_all if record_fast else n_full)
    assert [s[5] for s in everything].count(True) == (n_all - n_full if record_fast else 0)
    assert all(len(it) == (5 if record_fast else 4) for it in host.experience_buffer._items)
    # host and device replay batches, bit for bit
    bs = 6
    host.experience_buffer._rng = random.Random(9)
    dev.experience_buffer._rng = random.Random(9)
    bh = host._batch(host._sample(host.experience_buffer, bs))
    bd = dev._batch(dev._sample(dev.experience_buffer, bs))
    assert len(bh) == len(bd) == (4 if record_fast else 3)
    for u, v in zip(bh, bd):
        assert u.shape == v.shape and np.array_equal(pc.bits(u.numpy()), pc.bits(v.numpy()))
    if not record_fast:                              # today's expression
        with torch.no_grad():
            items = host.experience_buffer._items[:bs]
            x, pi, z = host._batch(items)
            assert torch.equal(host._loss(items)[0], F.cross_entropy(host.model(x)[0], pi))
        return
    assert set(bh[3].view(-1).tolist()) <= {0.0, 1.0} and tuple(bh[3].shape) == (bs, 1)
    # the weighted policy loss by hand: sum_i w_i CE_i / max(sum_i w_i, 1), CE_i the cross-entropy of row i alone.
    # Batches whose weighted sum is one f32 addition at most, so that the hand value is exact: none, one and two full rows.
    items = host.experience_buffer._items
    full = [it for it in items if it[4] == 1.0]
    fast = [it for it in items if it[4] == 0.0]
    assert len(full) >= 2 and len(fast) >= 3
    with torch.no_grad():
        def ce_of(it):
            x, pi, z, w = host._batch([it])
            out, _ = host.model(x)
            return F.cross_entropy(out, pi, reduction="none")[0]

        for batch, n_w in (([fast[0], fast[1], fast[2]], 0), ([fast[0], full[0], fast[1]], 1), ([full[1], fast[2], fast[0], full[0]], 2)):
            pl, vl = host._loss(batch)
            ces = [ce_of(it) for it in batch if it[4] == 1.0]
            if n_w == 0:
                assert float(pl) == 0.0
            elif n_w == 1:
                assert torch.equal(pl, ces[0])
            else:
                assert torch.equal(pl, (ces[0] + ces[1]) / 2)
            x, pi, z, w = host._batch(batch)
            assert torch.equal(vl, F.mse_loss(host.model(x)[1].squeeze(), z.squeeze()))                  # every row, as ever
        # the device path's loss on the same slots is the host's
        host.experience_buffer._rng = random.Random(4)
        dev.experience_buffer._rng = random.Random(4)
        lh = host._loss(host._sample(host.experience_buffer, bs))
        ld = dev._loss(dev._sample(dev.experience_buffer, bs))
        assert torch.equal(lh[0], ld[0]) and torch.equal(lh[1], ld[1])
    # and the optimiser loop runs on both
    host.experience_buffer._rng = random.Random(6)
    dev.experience_buffer._rng = random.Random(6)
    assert host.train() == dev.train() and host.history
