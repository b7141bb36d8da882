"""Training driver -- counterpart of the reference's AlphaZero class (src/py/alphazero.py:19-277)
without its wandb / pygame side channels.  Self-play runs on the engine (selfplay.play over
MCTS.search, whole search on the GPU when the model is a ResNet); the optimiser step stays plain
PyTorch(-ROCm):  loss = cross_entropy(policy_logits, pi) + mse(value, z)   (alphazero.py:200-209).

    az = AlphaZero(model, optimizer, FourPlayerChess, args, game_init_args)
    az.learn()

`args` takes the reference's keys (alphazero.py:291-306): max_game_length, C, num_searches,
num_iterations, num_games, num_parallel_games, batch_size, temperature, heuristic_weight,
replay_buffer_capacity, validation_buffer_capacity.  Beyond the reference: reuse_tree (default False) -- self-play keeps
the played move's subtree from ply to ply (play(); arena.py and the drop-in MCTS.search(games) never do);
device_replay (default False) -- both replay buffers live in device memory as fpc_tuple records
(replay_buffer.DeviceReplayBuffer): play() collects each ply's tuples on the device and pushes them into the rings
device to device, and every training batch is decoded by one kernel launch instead of one engine call per sample.
Same contents, entry for entry, and the same batches, bit for bit, as the host buffers give.  The rings belong to the
process-wide engine handle, which is therefore sized when this object is made and must not be re-created afterwards,
and which has one pair of rings: a second AlphaZero with device_replay in the same process takes them over (it empties
them), and the first one's next use of its buffers raises.
device_play (default False) -- each ply's moves are drawn, made and judged on the device by one launch
(fpc_ffi.Engine.search_play on the finished search) instead of a per-game numpy draw and two board-op round trips; the
draw is selfplay.sample_move's: the inverse CDF over pow(visits, 1/temperature) in f64, which picks sample_action's
child except within rounding of a boundary.  Composes with reuse_tree and device_replay.
refill (default False) -- learn() plays the num_games of an iteration as ONE run of num_parallel_games slots in which
a finished game's batch position is taken by a new game (play(total_games=num_games), selfplay.play(refill=...)) instead
of num_games // num_parallel_games runs that shrink to their longest game; with reuse_tree the rows that go on keep their
subtrees beside the fresh ones (fpc_search_advance_refill).  Composes with reuse_tree, device_play and device_replay.
sim_budget (default None; with reuse_tree) -- per-game simulation budgets for the plies that continue kept subtrees
(mcts.budgets_for, fpc_search_set_budget): "per_game" gives every game num_searches unless its own kept visits leave less
room, so a fresh row is no longer cut short by a kept root beside it; "visit_target" searches every root until
num_searches simulations have gone through it, kept ones included, and needs a handle of num_searches, not twice that.
solver (default False; with rules = "training" / "selfplay") -- the MCTS solver (fpc_search_set_solver): the search proves
wins, losses and draws up the tree, and play() plays a proven win or draw at every temperature -- on the host path from
fpc_search_proofs (selfplay.proven_pick), on the device_play path inside fpc_search_play.  arena.py does not use it.
forced_playouts (default None; a float, usually 2.0, with rules = "selfplay" and root_noise) -- forced playouts and policy
target pruning at the root (fpc_search_set_forced): the tuples and the move draw take the pruned visit counts, on the host
path from fpc_search_targets (selfplay.play(targets=True)), on the device paths inside fpc_collect_tuples / fpc_search_play.
playout_cap (default None; {"full_prob": p, "fast_searches": n, "record_fast": False}) -- playout cap randomization
(fpc_search_set_fast_rows): every ply every game draws a full search (probability p) or a fast one of n simulations without
noise, forcing or pruning.  record_fast False (the KataGo paper's way): a fast ply goes into neither buffer.  record_fast
True: it is stored with policy-loss weight 0 (the record's FPC_TUPLE_FAST flag on the device path, a fifth item element on
the host path) and _loss averages the policy cross-entropy over the full plies only; the value loss takes every row.
z_from_result (default False: the reference's labels, quirk Q12) -- a game that ends on the board labels its tuples by the
result (winner's team +1, the other -1, stalemate 0), the value rules = "training" backs up from a terminal leaf.
"""
import numpy as np
import torch
import torch.nn.functional as F

import alphazero_cpp as az
import selfplay
import tuples
from mcts import MCTS
from replay_buffer import DeviceReplayBuffer, ReplayBuffer


class AlphaZero:
    def __init__(self, model, optimizer, gameType, args, game_init_args=None, evaluator=None, seed=None):
        self.model, self.optimizer, self.gameType, self.args = model, optimizer, gameType, args
        self.game_init_args = game_init_args
        self.scheduler = torch.optim.lr_scheduler.StepLR(optimizer, step_size=1000, gamma=0.1)   # alphazero.py:25-27
        # args["fc_weights"] = "int8" (opt-in, fp16 engines): the self-play engine's policy Linear runs on int8 weights; MCTS reads
        # the key and every weight sync (host export or device pack) carries it
        self.mcts = MCTS(gameType, evaluator if evaluator is not None else model, args)
        self.device_replay = bool(args.get("device_replay", False)) if hasattr(args, "get") else False
        if self.device_replay:
            eng = self._engine()
            dev = None if eng.host_memory else "cuda"                 # None: the test-suite's emulator build writes host memory
            self.experience_buffer = DeviceReplayBuffer(eng, 0, args["replay_buffer_capacity"], device=dev)
            self.validation_buffer = DeviceReplayBuffer(eng, 1, args["validation_buffer_capacity"], device=dev)
        else:
            self.experience_buffer = ReplayBuffer(args["replay_buffer_capacity"])
            self.validation_buffer = ReplayBuffer(args["validation_buffer_capacity"])
        self.gen = torch.Generator().manual_seed(seed) if seed is not None else None
        cap = args.get("playout_cap", None) if hasattr(args, "get") else None
        self.playout_cap = None if cap is None else {"full_prob": self.mcts.playout_cap[0], "fast_searches": self.mcts.playout_cap[1]}
        self.record_fast = bool(cap.get("record_fast", False)) if hasattr(cap, "get") else False
        self.history = []

    # ---- self-play (alphazero.py:81-178) ----
    def _new_game(self):
        return self.gameType() if not self.game_init_args else self.gameType(*self.game_init_args)

    def _engine(self):
        G = int(self.args["num_parallel_games"])
        # same (rows = games x leaves_per_step, sims, dtype) request as MCTS.search makes, so the handle is not re-created under us
        # args["reuse_tree"] (opt-in, default off; not reference semantics): every ply after the first continues on the
        # subtree of the move played (MCTS.continue_search) -- with the internal network or an external evaluator alike.
        # The handle then holds 2 * num_searches simulations: the visits kept from the last ply count against max_sims
        # -- unless args["sim_budget"] = "visit_target" searches every root only up to num_searches simulations through
        # it (mcts.budgets_for): kept + new visits then never pass num_searches, and the handle holds just that
        reuse = bool(self.args.get("reuse_tree", False)) if hasattr(self.args, "get") else False
        double = reuse and self.mcts.sim_budget != "visit_target"
        return az.engine(self.mcts.engine_rows(G), int(self.args["num_searches"]) * (2 if double else 1), self.mcts.nn_dtype if self.mcts._native else None)

    def play(self, total_games=None):
        """One self-play run of num_parallel_games games; total_games (at least that many): the batch starts with
        num_parallel_games and every finished game's position is refilled with a new game until total_games have been
        started (selfplay.play(refill=...)); with reuse_tree the kept rows keep their subtrees beside the fresh ones."""
        G = int(self.args["num_parallel_games"])
        total = G if total_games is None else max(int(total_games), G)
        games = [self._new_game() for _ in range(total)]
        reuse = bool(self.args.get("reuse_tree", False)) if hasattr(self.args, "get") else False
        device_play = bool(self.args.get("device_play", False)) if hasattr(self.args, "get") else False
        eng = self._engine()
        L = int(self.args["max_game_length"])
        uniforms = torch.rand(L, total, generator=self.gen, dtype=torch.float64).tolist()
        # the cap's draws are a second block, made only when the cap is on: a seeded run without it is what it was
        cap_uniforms = torch.rand(L, total, generator=self.gen, dtype=torch.float64).tolist() if self.playout_cap is not None else None

        def search_fn(pods, fast=None):
            boards = [self.gameType._wrap(p) for p in pods]
            roots = self.mcts.search(boards, fast=fast)
            arrs = [r.child_arrays() for r in roots]                 # no Python object per child
            n = max(len(f) for f, _ in arrs)
            res = {"n_children": np.array([len(f) for f, _ in arrs]),
                   "flat": np.zeros((len(roots), n), np.int64), "visits": np.zeros((len(roots), n), np.int64)}
            for i, (f, v) in enumerate(arrs):
                res["flat"][i, :len(f)] = f
                res["visits"][i, :len(v)] = v
            return res

        def continue_fn(keep_idx, picks, pods, fast=None):
            return self.mcts.continue_search(pods, keep_idx, picks, fast=fast)

        where = {}                                        # device replay: (game id, loop step) -> index of the collected tuple

        def on_searched(ids, step):
            for g in ids:
                where[(g, step)] = len(where)
            eng.collect_tuples(ids, step)

        if self.device_replay:
            if eng is not self.experience_buffer.eng:
                raise RuntimeError("device_replay: the engine handle was re-created (alphazero_cpp.engine grew or was "
                                   "reconfigured) and the replay rings went with it")
            eng.tuples_reserve(L * total)
        episodes = selfplay.play(search_fn, eng, [g._b for g in games[:G]], self.args, uniforms, continue_fn=continue_fn if reuse else None,
                                 on_searched=on_searched if self.device_replay else None, device_play=device_play,
                                 refill=[g._b for g in games[G:]] if total > G else None,
                                 z_from_result=bool(self.args.get("z_from_result", False)) if hasattr(self.args, "get") else False,
                                 solver=self.mcts.solver_in_effect(), targets=self.mcts.forced_in_effect(),
                                 playout_cap=self.playout_cap, cap_uniforms=cap_uniforms)
        split = self.args["replay_buffer_capacity"] / (self.args["replay_buffer_capacity"] + self.args["validation_buffer_capacity"])
        if self.device_replay:
            z_team = np.zeros((2, len(episodes)), np.float32)      # z by (game, team of the side to move), as the Episodes have it
            src, ring_of = [], []
            for k, ep in enumerate(episodes):
                for ply, ((pod, _, _), z) in enumerate(zip(ep.entries, ep.z)):
                    z_team[pod.turn & 1, k] = z
                    if ep.fast[ply] and not self.record_fast:     # a fast ply is not stored: no index, no split draw
                        continue
                    src.append(where[(ep.gid, ep.start + ply)])
                    ring_of.append(0 if torch.rand(1, generator=self.gen).item() < split else 1)
            for k in range(0, len(episodes), eng.max_games):      # fpc_tuples_set_z takes max_games games per call
                eng.tuples_set_z([ep.gid for ep in episodes[k:k + eng.max_games]], z_team[0, k:k + eng.max_games], z_team[1, k:k + eng.max_games])
            eng.replay_push(src_index=src, ring_of=ring_of)
            return episodes
        for ep in episodes:                               # handle_terminal_state, alphazero.py:53-78
            for (pod, flats, visits), z, fast in zip(ep.entries, ep.z, ep.fast):
                if fast and not self.record_fast:             # a fast ply is not stored: no split draw
                    continue
                buf = self.experience_buffer if torch.rand(1, generator=self.gen).item() < split else self.validation_buffer
                if self.record_fast:
                    buf.add((pod, flats, visits, float(z), 0.0 if fast else 1.0))
                else:
                    buf.add((pod, flats, visits, float(z)))
        return episodes

    # ---- optimiser step (alphazero.py:181-258) ----
    def _batch(self, sample):
        if self.device_replay:                            # DeviceReplayBuffer.sample: the decoded batch itself
            dev = next(self.model.parameters()).device
            return tuple(t.to(dev) for t in sample)
        eng = az.engine()
        A = self.gameType.action_space_size
        dev = next(self.model.parameters()).device
        # GetEncodedState(entry.state) encodes each tuple on its own => per-sample rotation (alphazero.py:71-73)
        x = np.concatenate([eng.encode([s[0]]) for s in sample])
        pi = torch.stack([tuples.dense_pi({"flat": np.asarray(s[1], np.int64), "visits": np.asarray(s[2], np.int64)}, A) for s in sample])
        z = torch.tensor([s[3] for s in sample], dtype=torch.float32).view(-1, 1)
        if self.record_fast:
            w = torch.tensor([s[4] for s in sample], dtype=torch.float32).view(-1, 1)
            return torch.from_numpy(x).to(dev), pi.to(dev), z.to(dev), w.to(dev)
        return torch.from_numpy(x).to(dev), pi.to(dev), z.to(dev)

    def _sample(self, buf, bs):
        """a minibatch of `buf`; with record_fast the device buffer decodes the weight column too"""
        return buf.sample(bs, weights=True) if self.device_replay and self.record_fast else buf.sample(bs)

    def _loss(self, sample):
        batch = self._batch(sample)
        x, pi, z = batch[:3]
        out_policy, out_value = self.model(x)
        if self.record_fast:      # sum_i w_i CE_i / max(sum_i w_i, 1): the policy loss of the full plies alone
            w = batch[3].view(-1)
            ce = F.cross_entropy(out_policy, pi, reduction="none")
            policy_loss = (w * ce).sum() / torch.clamp(w.sum(), min=1.0)
        else:
            policy_loss = F.cross_entropy(out_policy, pi)
        value_loss = F.mse_loss(out_value.squeeze(), z.squeeze())
        return policy_loss, value_loss

    def train(self):
        bs = int(self.args["batch_size"])
        if len(self.experience_buffer) < bs:
            return None
        last = None
        for _ in range(0, len(self.experience_buffer), bs):
            policy_loss, value_loss = self._loss(self._sample(self.experience_buffer, bs))
            loss = policy_loss + value_loss
            self.optimizer.zero_grad()
            loss.backward()
            self.optimizer.step()
            self.scheduler.step()
            last = {"policy_loss": policy_loss.item(), "value_loss": value_loss.item(), "loss": loss.item()}
            self.history.append(last)
        return last

    @torch.no_grad()
    def validate(self):
        bs = int(self.args["batch_size"])
        if len(self.validation_buffer) < bs:
            return None
        policy_loss, value_loss = self._loss(self._sample(self.validation_buffer, bs))
        return {"policy_loss": policy_loss.item(), "value_loss": value_loss.item(), "loss": (policy_loss + value_loss).item()}

    def learn(self):                                      # alphazero.py:260-277
        for _ in range(int(self.args["num_iterations"])):
            self.model.eval()
            if bool(self.args.get("refill", False)) if hasattr(self.args, "get") else False:
                self.play(total_games=int(self.args["num_games"]))     # one full batch, refilled up to num_games
            else:
                for _ in range(int(self.args["num_games"]) // int(self.args["num_parallel_games"])):
                    self.play()
            self.model.train()
            self.train()
            self.model.eval()
            self.play()
            self.validate()
