"""LeagueArena: every agent of a pool against every other in ONE batch of cPongDouble, both bats served and every finished episode
booked per (left agent, right agent) pair on the device.

The reference plays one pair at a time: ``evaluate_two_policies_in_batch`` (pong/evaluate.py:6-88) takes two policies and the host walks
every step; the payoff matrix of a pool of A agents -- what snapshot selection, Elo or Nash ratings read -- is A * A such matches.  Here
each env holds a pair, the whole round-robin runs side by side, and the env's next pair is drawn inside the step:

* both seats are served by ONE ``crl_league`` of ``2 * num_envs`` virtual envs: virtual env ``2 * i + seat`` reads view ``seat`` of env
  ``i`` out of the env's ``(N, 2, K, 42, 42)`` observation buffer and writes ``actions[i, seat]``; its int32 ``[2N]`` assignment is the
  array of (left, right) pairs.  The launches are the league's own (one partition, one fill, one list launch per CNN agent for both
  seats together; three per pass for a full-size ActorCritic agent, ``add_full_agent``, whose snapshots enter the payoff matrix like
  any other agent).  That league is created with ``env_id_base = 2 * (the env's)``, so RANDOM's action stream is keyed by
  ``2 * gid + seat`` (``league_draw_reference(seed, 2 * gid + seat, step, CRL_LEAGUE_DOMAIN_ACTION, 3)``), and so is the stream of
  the agents' sampled and explored actions (``set_sampling``; ``league_sample_reference(seed, 2 * gid + seat, step, ...)``);
* the books and the pair draws are ``crl_arena_*`` (csrc/pong_arena.hip), an object beside the league as ``crl_ledger`` is:
  ``ArenaBooks`` below is its thin binding (device tensors in, device tensors out), ``LeagueArena`` ties it to an env and a league;
* nothing synchronises with the host unless the caller asks for host values (``counters()``, ``payoff()``, ``weights()``,
  ``state_dict()``, ``play()`` every ``check_every`` steps).

The rules are written down in include/crl.h ("arena books", "arena draws", "balance weights") and restated in numpy at the end of this
module (``arena_draw_reference``, ``balance_weights_reference``).  There is no torch model and no CPU path here.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N
from .league import (_BUILTIN_KINDS, _add_full, _full_weights, _get_sampling, _light_weights, _set_sampling, check_sampling,
                     league_draw_reference)
from .policy_serving import _KEYS, BUILTIN_CHECKPOINTS, load_light_weights
from .tournament import get_builtin_agent_names

_A = N.CRL_LEAGUE_MAX_AGENTS
_NC = N.CRL_ARENA_COUNTERS
NAMES = N.CRL_ARENA_COUNTER_NAMES


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class ArenaBooks:
    """Per-pair results of ``num_envs`` envs over a pool of ``agents`` agents, and the draw of pairs (``crl_arena_*``).  ``env_id_base``:
    the global id of env 0 (a shard passes its own, so that its draws are those of the whole batch); ``seed``: the key of the draws."""

    def __init__(self, num_envs, agents, device, seed=0, env_id_base=0):
        self.num_envs, self.agents = int(num_envs), int(agents)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("ArenaBooks lives on the GPU (there is no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if not 1 <= self.agents <= _A:
            raise ValueError(f"a pool holds 1 to {_A} agents, not {agents}")
        self.env_id_base = int(env_id_base)
        self._seed = int(seed) & (2 ** 64 - 1)
        self._L = N.load()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._L.crl_arena_create(self.device.index or 0, self.num_envs, self.env_id_base, self._seed, self.agents, C.byref(h)))
        self._h = h

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _pairs_ok(self, pairs, what):
        if pairs.dtype != torch.int32 or pairs.numel() != 2 * self.num_envs or not pairs.is_contiguous() or pairs.device != self.device:
            raise ValueError(f"{what}: pairs must be a contiguous int32 tensor of {self.num_envs} (left, right) rows on {self.device}")

    # ---- the step
    def update(self, pairs, reward, done, redraw=False, out=None):
        """One step of the books.  ``pairs`` int32 (N, 2) or (2N,): the (left, right) agents that PLAYED this step; ``reward`` float32
        (N,) or (N, k): the LEFT agent's step reward is column 0 (the env's own reward buffer can be passed as it is); ``done`` uint8
        (N,).  Returns int32 pairs of the shape of ``pairs`` (``out`` if given; it may be ``pairs``): the pairs played, with a fresh arena
        draw where ``done`` is set and ``redraw`` is true.  Device tensors in, device tensor out, no synchronisation."""
        n = self.num_envs
        self._pairs_ok(pairs, "update")
        if reward.dtype != torch.float32 or done.dtype != torch.uint8:
            raise TypeError("update(pairs int32, reward float32, done uint8): got %s, %s, %s" % (pairs.dtype, reward.dtype, done.dtype))
        if done.numel() != n or reward.shape[0] != n or not done.is_contiguous() or reward.dim() > 2:
            raise ValueError(f"update: a contiguous (N,) done and a reward of N rows with the left agent's reward in column 0, N = {n}")
        stride = reward.stride(0) if n > 1 else 1
        if out is None:
            out = torch.empty_like(pairs)
        else:
            self._pairs_ok(out, "update (out)")
        N.check(self._L.crl_arena_step(self._h, _p(pairs), _p(reward), stride, _p(done), int(bool(redraw)), _p(out), self._stream()))
        return out

    def draw(self, pairs, out=None):
        """A fresh arena draw for EVERY env (each env's draw counter moves by one); with a table that sums to 0 ``pairs`` comes back."""
        self._pairs_ok(pairs, "draw")
        if out is None:
            out = torch.empty_like(pairs)
        else:
            self._pairs_ok(out, "draw (out)")
        N.check(self._L.crl_arena_draw(self._h, _p(pairs), _p(out), self._stream()))
        return out

    # ---- results
    def _counters_and_ignored(self):
        both = torch.empty((_NC * _A * _A + 1,), dtype=torch.int64, device=self.device)
        N.check(self._L.crl_arena_get_counters(self._h, _p(both), C.c_void_p(both.data_ptr() + 8 * _NC * _A * _A), self._stream()))
        return both

    def counters_device(self):
        """int64 (6, 16, 16) device tensor, planes in the order of ``_native.CRL_ARENA_COUNTER_NAMES``, indexed [left][right]: a copy,
        enqueued on the current stream (no synchronisation).  The shape ``balance_weights(counters=...)`` takes, e.g. after an
        all-reduce."""
        out = torch.empty((_NC, _A, _A), dtype=torch.int64, device=self.device)
        N.check(self._L.crl_arena_get_counters(self._h, _p(out), None, self._stream()))
        return out

    def counters(self):
        """Host dict: the six int64 (agents, agents) arrays (``episodes``, ``left_wins``, ``right_wins``, ``draws``, ``return_sum``,
        ``length_sum``; [left][right], cut to the pool) and ``ignored`` (episodes with an id outside the pool).  SYNCHRONISES."""
        host = self._counters_and_ignored().cpu().numpy()
        planes = host[:-1].reshape(_NC, _A, _A)
        d = {k: planes[i, :self.agents, :self.agents].copy() for i, k in enumerate(NAMES)}
        d["ignored"] = int(host[-1])
        return d

    def env_state(self):
        """Device tensors (ret int32, len int32, draw_ctr as int32 bits) of the running episodes: copies, no synchronisation."""
        t = [torch.empty((self.num_envs,), dtype=torch.int32, device=self.device) for _ in range(3)]
        N.check(self._L.crl_arena_get_env_state(self._h, _p(t[0]), _p(t[1]), _p(t[2]), self._stream()))
        return tuple(t)

    # ---- weights
    def set_agents(self, agents):
        """The pool grew: the cells of a new agent enter the table with weight 1 (0 on the diagonal), only the weight table changes: the counters of
        those cells are what they were (zero unless the pool held them before or ``load_state_dict`` wrote them)."""
        N.check(self._L.crl_arena_set_agents(self._h, int(agents), self._stream()))
        self.agents = int(agents)

    def set_weights(self, weights):
        """``weights``: (agents, agents) non-negative integers [left][right] (host values); their sum must lie in [1, 2^32).  A cell of
        weight 0 is never drawn."""
        w = np.asarray(weights)
        if w.shape != (self.agents, self.agents) or (w < 0).any() or (w > 0xFFFFFFFF).any():
            raise ValueError(f"set_weights: ({self.agents}, {self.agents}) integers in [0, 2^32)")
        w = np.ascontiguousarray(w, np.uint32)
        N.check(self._L.crl_arena_set_weights(self._h, w.ctypes.data_as(C.c_void_p), w.size, self._stream()))

    def balance_weights(self, include_mirror=False, floor=1, counters=None):
        """Fills the table on the device: weight = floor + min(most episodes of a scheduled cell - this cell's, 65535) for the scheduled
        cells (the pool's, without the diagonal unless ``include_mirror``), 0 elsewhere.  ``counters``: an int64 (6, 16, 16) device
        tensor in place of the arena's own (a sharded caller passes the all-reduced ``counters_device()``).  No synchronisation."""
        if counters is not None:
            if counters.dtype != torch.int64 or tuple(counters.shape) != (_NC, _A, _A) or not counters.is_contiguous() or counters.device != self.device:
                raise ValueError(f"balance_weights: counters must be a contiguous int64 ({_NC}, {_A}, {_A}) tensor on {self.device}")
        N.check(self._L.crl_arena_balance_weights(self._h, _p(counters), int(bool(include_mirror)), int(floor), self._stream()))

    def weights_device(self):
        """int64 (16, 16) device tensor holding the uint32 table (cells beyond the pool are 0): a copy, no synchronisation."""
        raw = torch.empty((_A, _A), dtype=torch.int32, device=self.device)
        N.check(self._L.crl_arena_get_weights(self._h, _p(raw), self._stream()))
        return raw.to(torch.int64) & 0xFFFFFFFF

    def weights(self):
        """The table of the pool as a host uint32 (agents, agents) array (synchronises)."""
        return self.weights_device()[:self.agents, :self.agents].cpu().numpy().astype(np.uint32)

    # ---- lifetime
    def seed(self, s):
        """New key for the draws; every env's draw counter starts over.  Results and weights stay."""
        self._seed = int(s or 0) & (2 ** 64 - 1)
        N.check(self._L.crl_arena_seed(self._h, self._seed, self._stream()))

    def reset(self):
        """Zeroes the counters and the running returns / lengths (weights, key and draw counters stay)."""
        N.check(self._L.crl_arena_reset(self._h, self._stream()))

    def state_dict(self):
        """Everything a continuation needs, as host arrays (synchronises)."""
        both = self._counters_and_ignored().cpu().numpy()
        ret, length, ctr = self.env_state()
        return {"agents": self.agents, "seed": self._seed, "counters": both[:-1].reshape(_NC, _A, _A).copy(), "ignored": int(both[-1]),
                "ret": ret.cpu().numpy(), "len": length.cpu().numpy(), "draw_ctr": ctr.cpu().numpy().view(np.uint32), "weights": self.weights()}

    def load_state_dict(self, sd):
        if int(sd["agents"]) != self.agents or len(sd["ret"]) != self.num_envs:
            raise ValueError(f"load_state_dict: books of {sd['agents']} agents x {len(sd['ret'])} envs into ones of {self.agents} x {self.num_envs}")
        w, counters = np.asarray(sd["weights"]), np.asarray(sd["counters"], np.int64)
        if counters.size != _NC * _A * _A or w.shape != (self.agents, self.agents):
            raise ValueError(f"load_state_dict: counters of ({_NC}, {_A}, {_A}) and weights of ({self.agents}, {self.agents}) are needed")
        if not w.any() and self.weights().any():  # (looked at before anything is written)
            raise ValueError("load_state_dict: an all-zero weight table cannot be set (crl_arena_set_weights refuses a sum of 0)")
        self.seed(sd["seed"])  # (zeroes the draw counters; they are written below)
        both = torch.from_numpy(np.concatenate([counters.reshape(-1), [np.int64(sd["ignored"])]])).to(self.device)
        N.check(self._L.crl_arena_set_counters(self._h, _p(both), C.c_void_p(both.data_ptr() + 8 * _NC * _A * _A), self._stream()))
        t = [torch.from_numpy(np.ascontiguousarray(sd[k]).view(np.int32).copy()).to(self.device) for k in ("ret", "len", "draw_ctr")]
        N.check(self._L.crl_arena_set_env_state(self._h, _p(t[0]), _p(t[1]), _p(t[2]), self._stream()))
        if w.any():
            self.set_weights(w)
        torch.cuda.current_stream(self.device).synchronize()  # the staging tensors above are this call's own

    def close(self):
        if getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            self._L.crl_arena_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.crl_arena_destroy(self._h)
                self._h = None
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


class LeagueArena:
    """The round-robin of a pool on one ``cPongDouble-v0`` batch.  ``env``: a ``HipPongVecEnv`` in wrapped mode with ``resized_dim=42``
    and uint8 observations (``make_envs("cPongDouble-v0", ..., resized_dim=42, frame_stack=None)``).  ``agent_names``: any of RANDOM,
    RULE_BASED, WEAK, MEDIUM (default: all four); ``add_agent`` adds LightActorCritic weight sets of the caller's own, ``add_full_agent``
    full-size ActorCritic ones.
    ``env_id_base``: the global id of env 0 (default: the env's); the pair draws are keyed by that REAL id, the league that serves the
    bats is created with twice it, so RANDOM's action stream and the sample stream of ``set_sampling`` are keyed by ``2 * gid + seat``.
    ``include_mirror``: schedule an agent
    against itself too.  After construction env with global id g holds the (g mod cells)-th scheduled pair in row-major order;
    ``draw_pairs()`` replaces that by arena draws."""

    def __init__(self, env, num_envs, agent_names=None, seed=0, env_id_base=None, include_mirror=False):
        from .vec_env import HipPongVecEnv

        ok = (isinstance(env, HipPongVecEnv) and not env.single and env.mode == "wrapped" and env.R == 42 and env._buf_dtype == torch.uint8
              and env.output == "torch")
        if not ok:
            raise ValueError('LeagueArena takes the HIP cPongDouble-v0 vector env in wrapped mode with resized_dim=42 and uint8 observations: '
                             'pass make_envs("cPongDouble-v0", num_envs=N, resized_dim=42, frame_stack=None, log_dir=None)')
        if int(num_envs) != env.num_envs:
            raise ValueError(f"num_envs = {num_envs}, but the env holds {env.num_envs}")
        self.env, self.num_envs = env, int(num_envs)
        self.device = env.device
        self.include_mirror = bool(include_mirror)
        self.redraw_on_done = True
        self.record_logits = False  # tests: keep the CNN agents' logits of every step (``logits()``)
        self.env_id_base = int(env.env_id_base if env_id_base is None else env_id_base)
        self._seed = int(seed) & (2 ** 64 - 1)
        self._plane = 42 * 42
        self._L = N.load()
        n2 = 2 * self.num_envs
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._L.crl_league_create(self.device.index or 0, n2, 2 * self.env_id_base, self._seed, C.byref(h)))
        self._h = h
        self.agent_names, self._kinds = [], []
        self._act = torch.zeros((self.num_envs, 2), dtype=torch.int32, device=self.device)
        self._logits = torch.zeros((n2, 3), dtype=torch.float32, device=self.device)
        self._pairs = torch.zeros((self.num_envs, 2), dtype=torch.int32, device=self.device)  # the league's assignment, kept beside it
        self._buf = None  # the observation buffer both seats act on: the previous step's / the reset's
        names = get_builtin_agent_names() if agent_names is None else list(agent_names)
        for name in names:
            if name in _BUILTIN_KINDS:
                self._add(name, _BUILTIN_KINDS[name], None)
            elif name in BUILTIN_CHECKPOINTS:
                self._add(name, N.CRL_LEAGUE_LIGHT, load_light_weights(BUILTIN_CHECKPOINTS[name]))
            else:
                raise ValueError("Unknown agent name: {}".format(name))
        if not self.agent_names:
            raise ValueError("the pool is empty")
        self.books = ArenaBooks(self.num_envs, len(self.agent_names), self.device, seed=self._seed, env_id_base=self.env_id_base)
        cells = self.scheduled().nonzero()
        if len(cells[0]) == 0:  # one agent and no mirror matches: nothing is scheduled, the agent plays itself
            cells = (np.zeros(1, np.int64), np.zeros(1, np.int64))
        k = (self.env_id_base + np.arange(self.num_envs)) % len(cells[0])
        self.set_pairs(cells[0][k], cells[1][k])

    # ---- pool
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _add(self, name, kind, weights):
        if name in self.agent_names:
            raise ValueError(f"{name} is in the pool already")
        if len(self.agent_names) >= _A:
            raise ValueError(f"a pool holds at most {_A} agents")
        with torch.cuda.device(self.device):
            if kind == N.CRL_LEAGUE_LIGHT:
                N.check(self._L.crl_league_add_light(self._h, *[weights[k].ctypes.data_as(C.c_void_p) for k in _KEYS]))
            else:
                N.check(self._L.crl_league_add_builtin(self._h, kind))
        self.agent_names.append(name)
        self._kinds.append(kind)

    def add_agent(self, name, weights_or_checkpoint, temperature=0.0, epsilon=0.0):
        """A LightActorCritic agent of one's own -- a checkpoint path, a dict of the six arrays in torch layout or a light ``Policy``
        (a trainer's snapshot).  Its cells enter the draw table with weight 1; the pairs in force stay.  Full-size networks are refused
        here: ``add_full_agent`` takes them.
        ``temperature`` / ``epsilon``: its play style (``set_sampling``); the default is greedy."""
        check_sampling(temperature, epsilon)  # (before the agent enters the pool)
        self._add(name, N.CRL_LEAGUE_LIGHT, _light_weights(name, weights_or_checkpoint))
        if temperature or epsilon:
            self.set_sampling(name, temperature, epsilon)
        self.books.set_agents(len(self.agent_names))

    def add_full_agent(self, name, weights_or_checkpoint, temperature=0.0, epsilon=0.0, scratch_rows=None):
        """A full-size ActorCritic agent of one's own (``LeagueEnvWrapper.add_full_agent``: a checkpoint path, a dict of the eight arrays
        in torch layout or a full-size ``Policy``), served in both seats.  Its cells enter the draw table with weight 1; the pairs in
        force stay.  ``scratch_rows``: rows of the one activation scratch (None: min(2 * num_envs, 65 536) -- the seats are the rows)."""
        check_sampling(temperature, epsilon)  # (before the agent enters the pool)
        _add_full(self, name, _full_weights(name, weights_or_checkpoint), scratch_rows)
        if temperature or epsilon:
            self.set_sampling(name, temperature, epsilon)
        self.books.set_agents(len(self.agent_names))

    def set_sampling(self, agent, temperature=1.0, epsilon=0.0):
        """The play style of ``agent`` (a name or an index) in either seat, from the next step on (``LeagueEnvWrapper.set_sampling``):
        temperature 0 plays the argmax, T > 0 samples from softmax(logits / T); epsilon is the share of uniform actions."""
        _set_sampling(self, agent, temperature, epsilon)

    def sampling(self):
        """Host dict ``name -> (temperature, epsilon)`` of the whole pool (no GPU work)."""
        return _get_sampling(self)

    def get_agent_names(self):
        return self.agent_names

    def scheduled(self):
        """bool (agents, agents): the cells the arena schedules -- every pair of the pool, the diagonal only with ``include_mirror``."""
        a = len(self.agent_names)
        return np.ones((a, a), bool) if self.include_mirror else ~np.eye(a, dtype=bool)

    # ---- pairs
    def _ids(self, x, what):
        if isinstance(x, str):
            if x not in self.agent_names:
                raise ValueError(f"{what}: {x} is not in the pool {self.agent_names}")
            x = self.agent_names.index(x)
        t = torch.as_tensor(x).to(self.device, torch.int32).reshape(-1)
        if t.numel() == 1:
            t = t.expand(self.num_envs)
        if t.numel() != self.num_envs:
            raise ValueError(f"{what}: one agent for all envs or one per env ({self.num_envs}), got {t.numel()}")
        return t

    def set_pairs(self, left, right):
        """``left`` / ``right``: an agent name or index for every env, or one index per env ((N,) array / tensor)."""
        both = torch.stack([self._ids(left, "left"), self._ids(right, "right")], 1).contiguous()
        if int(both.min()) < 0 or int(both.max()) >= len(self.agent_names):
            raise ValueError(f"agent ids must index agent_names (0..{len(self.agent_names) - 1})")
        self._pairs.copy_(both)
        N.check(self._L.crl_league_set_assignment(self._h, _p(self._pairs), 0, self._stream()))

    @property
    def pairs(self):
        """int32 (N, 2) device tensor: a copy of the (left, right) pairs in force (no synchronisation)."""
        return self._pairs.clone()

    def draw_pairs(self):
        """A fresh arena draw for every env, on the device (no synchronisation)."""
        self.books.draw(self._pairs, out=self._pairs)
        N.check(self._L.crl_league_set_assignment(self._h, _p(self._pairs), 0, self._stream()))

    # ---- weights and results: the books'
    def set_weights(self, weights):
        self.books.set_weights(weights)

    def balance_weights(self, floor=1, counters=None):
        """Pairs that were played less are drawn more (``ArenaBooks.balance_weights`` over this arena's schedule)."""
        self.books.balance_weights(self.include_mirror, floor, counters)

    def weights(self):
        return self.books.weights()

    def counters_device(self):
        return self.books.counters_device()

    def counters(self):
        return self.books.counters()

    def payoff(self):
        """Host arrays (synchronises), nan where a pair has not been played: ``win_rate[l, r]`` = (left_wins + draws / 2) / episodes of
        the LEFT agent l against r on the right, ``mean_return`` (the left agent's), ``mean_length``, and the seat-symmetrised
        ``score[a, b]``: a's results against b over both seat orders, so that score[a, b] + score[b, a] = 1."""
        return payoff_from_counters(self.counters())

    def play(self, episodes_per_pair, max_steps, check_every=256, rebalance=True):
        """Steps until every scheduled cell holds at least ``episodes_per_pair`` episodes or ``max_steps`` steps are done.  The counters
        are read (a synchronisation) every ``check_every`` steps only, where ``balance_weights()`` is called as well.  Returns
        ``payoff()``.  The schedule is filled by the redraws at episode ends: with ``redraw_on_done`` off the envs keep their pairs and a
        cell that no env holds would never be played, so that combination is refused."""
        if not self.redraw_on_done:
            raise ValueError("play() fills the schedule through the redraws at episode ends: set redraw_on_done = True")
        if self._buf is None:
            self.reset()
        sched, t = self.scheduled(), 0
        while t < int(max_steps):
            self.step_device()
            t += 1
            if t % int(check_every) == 0 or t == int(max_steps):
                if (self.counters()["episodes"][sched] >= int(episodes_per_pair)).all():
                    break
                if rebalance:
                    self.balance_weights()
        return self.payoff()

    # ---- the step
    def logits(self):
        """float32 (2N, 3), row 2 * i + seat: with ``record_logits`` set, the logits of the last step for seats held by a CNN agent."""
        return self._logits

    @property
    def last_actions(self):
        """int32 (N, 2) device tensor: the actions of the step just played, [:, 0] the left bat's."""
        return self._act

    def _fill_actions(self):
        if self._buf is None:
            raise RuntimeError("reset() the arena before its first step")
        k = self.env.K
        N.check(self._L.crl_league_act(self._h, C.c_void_p(self._buf.data_ptr() + (k - 1) * self._plane), k * self._plane, _p(self._act), 1,
                                       _p(self._logits) if self.record_logits else None, self._stream()))
        return self._act

    def _after_step(self, rew, done):
        self.books.update(self._pairs, rew, done, redraw=self.redraw_on_done, out=self._pairs)
        if self.redraw_on_done:
            N.check(self._L.crl_league_set_assignment(self._h, _p(self._pairs), 0, self._stream()))

    def step_device(self):
        """Hot-loop entry (no host work, no synchronisation): both bats act on the previous observation buffer, the env steps, the step
        is booked and the envs whose episode ended get their next pair.  Returns the env's device buffers (obs (N, 2, K, 42, 42),
        rewards (N, 2), done (N,)) like ``HipPongVecEnv.step_device``."""
        buf, rew, done = self.env.step_device(self._fill_actions())
        self._buf = buf
        self._after_step(rew, done)
        return buf, rew, done

    def step(self):
        """``step_device`` with the env's host-friendly returns: (obs tuple, rewards (N, 2), dones, infos) of ``HipPongVecEnv.step``."""
        obs, rew, done, info = self.env.step(self._fill_actions())
        self._buf = self.env._obs[self.env._flip ^ 1]  # the buffer the step drew into
        self._after_step(self.env._rew, self.env._done)
        return obs, rew, done, info

    def reset(self, **kwargs):
        views = self.env.reset(**kwargs)
        self._buf = self.env._obs[self.env._flip ^ 1]  # the buffer the reset drew into
        return views

    # ---- lifetime
    def reset_history(self):
        """Zeroes the frame rings of both seats (``Policy.reset``)."""
        N.check(self._L.crl_league_reset(self._h, self._stream()))

    def seed(self, s):
        """Seeds the env and re-keys RANDOM's actions, the sampled and explored actions and the pair draws (all draw counters start over)."""
        self._seed = int(s or 0) & (2 ** 64 - 1)
        self.env.seed(s)
        N.check(self._L.crl_league_seed(self._h, self._seed, self._stream()))
        self.books.seed(s)

    def state_dict(self):
        """The arena's own state as host arrays (synchronises): the books, the pairs, both seats' frame rings and the observation
        buffer the next step acts on, and the pool's play styles (``sampling``: [temperature, epsilon] rows in pool order).  The env's
        state is the env's (``env.state_dict()``).  RANDOM's action counter is the league's -- it is the counter of the sampled and
        explored actions too -- and starts over with ``load_state_dict``: a pool with RANDOM, or with an agent that samples or explores,
        continues with other such actions than the original run."""
        stack = torch.empty((2 * self.num_envs, 4, 42, 42), dtype=torch.uint8, device=self.device)
        N.check(self._L.crl_league_get_stack(self._h, _p(stack), self._stream()))
        return {"agent_names": list(self.agent_names), "books": self.books.state_dict(), "pairs": self._pairs.cpu().numpy(),
                "stack": stack.cpu().numpy(), "obs": None if self._buf is None else self._buf.cpu().numpy(), "redraw_on_done": self.redraw_on_done,
                "sampling": np.array([self.sampling()[n] for n in self.agent_names], np.float32).reshape(-1, 2)}

    def load_state_dict(self, sd):
        if list(sd["agent_names"]) != self.agent_names:
            raise ValueError(f"load_state_dict: a pool of {list(sd['agent_names'])} into one of {self.agent_names}")
        # everything is looked at before anything is written: a refused load leaves the arena as it was
        books, p, stack, obs = sd["books"], np.asarray(sd["pairs"]), np.asarray(sd["stack"]), sd.get("obs")
        if int(books["agents"]) != self.books.agents or len(books["ret"]) != self.num_envs:
            raise ValueError(f"load_state_dict: books of {books['agents']} agents x {len(books['ret'])} envs into ones of "
                             f"{self.books.agents} x {self.num_envs}")
        if p.shape != (self.num_envs, 2) or p.min() < 0 or p.max() >= len(self.agent_names):
            raise ValueError(f"load_state_dict: pairs must be ({self.num_envs}, 2) ids that index agent_names")
        if stack.shape != (2 * self.num_envs, 4, 42, 42):
            raise ValueError(f"load_state_dict: frame rings of shape {stack.shape}, this arena's are {(2 * self.num_envs, 4, 42, 42)}")
        if obs is not None and tuple(np.shape(obs)) != tuple(self.env._obs_shape):
            raise ValueError(f"load_state_dict: an observation buffer of shape {tuple(np.shape(obs))} into an env of {self.env._obs_shape}")
        if not np.asarray(books["weights"]).any() and self.books.weights().any():
            raise ValueError("load_state_dict: an all-zero weight table cannot be set (crl_arena_set_weights refuses a sum of 0)")
        styles = None  # (a state dict from before the play styles leaves them as they are)
        if sd.get("sampling") is not None:
            styles = np.asarray(sd["sampling"], np.float32)
            if styles.shape != (len(self.agent_names), 2):
                raise ValueError(f"load_state_dict: sampling must hold a (temperature, epsilon) row per agent, got shape {styles.shape}")
            for t, e in styles:
                check_sampling(t, e)
        self._seed = int(books["seed"])
        N.check(self._L.crl_league_seed(self._h, self._seed, self._stream()))
        if styles is not None:
            for a, (t, e) in enumerate(styles):
                self.set_sampling(a, float(t), float(e))
        self.books.load_state_dict(books)
        self.set_pairs(p[:, 0], p[:, 1])
        stack = torch.from_numpy(np.ascontiguousarray(stack, np.uint8)).to(self.device)
        N.check(self._L.crl_league_set_stack(self._h, _p(stack), self._stream()))
        torch.cuda.current_stream(self.device).synchronize()
        if obs is not None:  # (a copy of the arena's own: the env's buffers are drawn again by its next step)
            self._buf = torch.from_numpy(np.ascontiguousarray(obs, np.uint8)).to(self.device)
        self.redraw_on_done = bool(sd["redraw_on_done"])

    def close(self):
        if getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            self._L.crl_league_destroy(self._h)
            self._h = None
            self.books.close()
            self.env.close()

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.crl_league_destroy(self._h)
                self._h = None
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def payoff_from_counters(c):
    """``LeagueArena.payoff`` from a ``counters()`` dict (host arithmetic)."""
    e, lw, rw, d = (np.asarray(c[k], np.int64) for k in ("episodes", "left_wins", "right_wins", "draws"))
    with np.errstate(invalid="ignore", divide="ignore"):
        ef = np.where(e > 0, e, np.nan).astype(np.float64)
        out = {"episodes": e.copy(), "win_rate": (lw + 0.5 * d) / ef, "mean_return": np.asarray(c["return_sum"], np.int64) / ef,
               "mean_length": np.asarray(c["length_sum"], np.int64) / ef}
        both = e + e.T
        # a's wins over b: as left against b, and as right when b sat left; halves of the draws of both seat orders.  In halves, as
        # integers: the two triangles then divide numbers that add up to the denominator exactly
        halves = 2 * (lw + rw.T) + (d + d.T)
        upper = halves / np.where(both > 0, 2 * both, np.nan).astype(np.float64)
        score = np.where(np.triu(np.ones_like(e, dtype=bool)), upper, 1.0 - upper.T)
        np.fill_diagonal(score, np.where(np.diag(e) > 0, 0.5, np.nan))
    out["score"] = score
    return out


def arena_draw_reference(seed, gid, counter, weights):
    """The arena's pair draw in numpy (include/crl.h "arena draws"): x = Philox4x32-10 word 0 of counter (gid lo, gid hi, counter,
    CRL_ARENA_DOMAIN_PAIR) under the seed; r = (x * T) >> 32 with T the sum of the table; the smallest row-major cell whose cumulative
    weight exceeds r.  ``weights``: (A, A) [left][right], A <= 16.  Arrays broadcast; returns int64 (left, right).  Host code for tests
    and for callers that want to predict a draw; the kernels do not use it."""
    w = np.asarray(weights)
    if w.ndim != 2 or w.shape[0] != w.shape[1] or not 1 <= w.shape[0] <= _A or (w < 0).any():
        raise ValueError(f"a square table of 1 to {_A} agents with non-negative weights")
    total = int(w.astype(np.uint64).sum())
    if not 0 < total < 2 ** 32:
        raise ValueError(f"the weights must sum to a value in [1, 2^32), not {total}")
    r = league_draw_reference(seed, gid, counter, N.CRL_ARENA_DOMAIN_PAIR, total)  # (x * T) >> 32
    cell = np.searchsorted(np.cumsum(w.astype(np.int64).reshape(-1)), r, side="right").astype(np.int64)  # (row-major within the pool)
    return cell // w.shape[0], cell % w.shape[0]


def balance_weights_reference(counters, agents, include_mirror=False, floor=1):
    """The balance table in numpy (include/crl.h "balance weights"), exactly what the device kernel writes.  ``counters``: int64
    (6, 16, 16) in the order of ``_native.CRL_ARENA_COUNTER_NAMES`` (only ``episodes`` is read).  Returns uint32 (16, 16); cells that
    are not scheduled are 0."""
    e = np.asarray(counters, np.int64).reshape(_NC, _A, _A)[0]
    a = int(agents)
    sched = np.zeros((_A, _A), bool)
    sched[:a, :a] = True
    if not include_mirror:
        sched &= ~np.eye(_A, dtype=bool)
    w = np.zeros((_A, _A), np.uint32)
    if sched.any():
        m = e[sched].max()
        w[sched] = (np.int64(floor) + np.minimum(m - e[sched], 65535)).astype(np.uint32)
    return w
