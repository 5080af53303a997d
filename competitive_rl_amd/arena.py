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
* the books and the pair draws are ``crl_arena_*`` (csrc/pong_arena.hip over csrc/pong_books.h, the core it shares with ``crl_ledger``),
  an object beside the league as ``crl_ledger`` is: ``ArenaBooks`` below is its thin binding (device tensors in, device tensors out;
  ``DeviceBooks`` of books.py with the pair as key), ``LeagueArena`` ties it to an env and the agent pool of league.py;
* nothing synchronises with the host unless the caller asks for host values (``counters()``, ``payoff()``, ``weights()``,
  ``state_dict()``, ``play()`` every ``check_every`` steps) or hands over ids of its own (``set_pairs`` checks their range on the host).

The rules are written down in include/crl.h ("arena books", "arena draws", "balance weights") and restated in numpy at the end of this
module (``arena_draw_reference``, ``balance_weights_reference``).  There is no torch model and no CPU path here.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N
from .books import DeviceBooks, _p
from .league import AgentPool, _full_weights, _light_weights  # noqa: F401  (the weight-set checks are re-exported)
from .rules import check_sampling, league_draw_reference
from .vec_env import HipPongVecEnv

_A = N.CRL_LEAGUE_MAX_AGENTS
_NC = N.CRL_ARENA_COUNTERS
NAMES = N.CRL_ARENA_COUNTER_NAMES


class ArenaBooks(DeviceBooks):
    """Per-pair results of ``num_envs`` envs over a pool of ``agents`` agents, and the draw of pairs (``DeviceBooks`` keyed by the cell
    [left][right]): counter planes int64 (6, 16, 16) in the order of ``_native.CRL_ARENA_COUNTER_NAMES`` (``episodes``, ``left_wins``,
    ``right_wins``, ``draws``, ``return_sum``, ``length_sum``); an (agents, agents) weight table."""

    _C, _NAMES, _PLANE = "crl_arena_", NAMES, (_A, _A)

    def _pairs_ok(self, pairs, what):
        if pairs.dtype != torch.int32 or pairs.numel() != 2 * self.num_envs or not pairs.is_contiguous() or pairs.device != self.device:
            raise ValueError(f"{what}: pairs must be a contiguous int32 tensor of {self.num_envs} (left, right) rows on {self.device}")

    def _out(self, pairs, out, what):
        self._pairs_ok(pairs, what)
        if out is None:
            return torch.empty_like(pairs)
        self._pairs_ok(out, what + " (out)")
        return out

    def update(self, pairs, reward, done, redraw=False, out=None):
        """One step of the books.  ``pairs`` int32 (N, 2) or (2N,): the (left, right) agents that PLAYED this step; ``reward`` float32
        (N,) or (N, k): the LEFT agent's step reward is column 0 (the env's own reward buffer can be passed as it is); ``done`` uint8
        (N,).  Returns int32 pairs of the shape of ``pairs`` (``out`` if given; it may be ``pairs``): the pairs played, with a fresh arena
        draw where ``done`` is set and ``redraw`` is true.  Device tensors in, device tensor out, no synchronisation."""
        return self._step(pairs, reward, done, redraw, self._out(pairs, out, "update"))

    def draw(self, pairs, out=None):
        """A fresh arena draw for EVERY env (each env's draw counter moves by one); with a table that sums to 0 ``pairs`` comes back."""
        out = self._out(pairs, out, "draw")
        N.check(self._L.crl_arena_draw(self._h, _p(pairs), _p(out), self._stream()))
        return out

    def balance_weights(self, include_mirror=False, floor=1, counters=None):
        """Fills the table on the device: weight = floor + min(most episodes of a scheduled cell - this cell's, 65535) for the scheduled
        cells (the pool's, without the diagonal unless ``include_mirror``), 0 elsewhere.  ``counters``: an int64 (6, 16, 16) device
        tensor in place of the arena's own (a sharded caller passes the all-reduced ``counters_device()``).  No synchronisation."""
        self._check_counters(counters, "balance_weights")
        N.check(self._L.crl_arena_balance_weights(self._h, _p(counters), int(bool(include_mirror)), int(floor), self._stream()))


class LeagueArena(AgentPool):
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
        n2 = 2 * self.num_envs
        self._act = torch.zeros((self.num_envs, 2), dtype=torch.int32, device=self.device)
        self._logits = torch.zeros((n2, 3), dtype=torch.float32, device=self.device)
        self._pairs = torch.zeros((self.num_envs, 2), dtype=torch.int32, device=self.device)  # the league's assignment, kept beside it
        self._buf = None  # the observation buffer both seats act on: the previous step's / the reset's
        self._open_pool(n2, 2 * self.env_id_base, self._seed, agent_names)  # the seats are the pool's rows
        self.books = ArenaBooks(self.num_envs, len(self.agent_names), self.device, seed=self._seed, env_id_base=self.env_id_base)
        cells = self.scheduled().nonzero()
        if len(cells[0]) == 0:  # one agent and no mirror matches: nothing is scheduled, the agent plays itself
            cells = (np.zeros(1, np.int64), np.zeros(1, np.int64))
        k = (self.env_id_base + np.arange(self.num_envs)) % len(cells[0])
        self.set_pairs(cells[0][k], cells[1][k])

    # ---- pool: the hook (``add_agent`` / ``add_full_agent`` / ``set_sampling`` are ``AgentPool``'s; a full-size agent is served in both seats)
    def _pool_grew(self):
        self.books.set_agents(len(self.agent_names))

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
        """``left`` / ``right``: an agent name or index for every env, or one index per env ((N,) array / tensor).  The ids are
        range-checked on the host, which synchronises with the current stream: not for the hot loop (``draw_pairs`` is)."""
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
    def seed(self, s):
        """Seeds the env and re-keys RANDOM's actions, the sampled and explored actions and the pair draws (all draw counters start over)."""
        self._seed = int(s or 0) & (2 ** 64 - 1)
        self.env.seed(s)
        self._seed_pool(s)
        self.books.seed(s)

    def state_dict(self):
        """The arena's own state as host arrays (synchronises): the books, the pairs, both seats' frame rings and the observation
        buffer the next step acts on, the pool's play styles (``sampling``: [temperature, epsilon] rows in pool order) and ``pool``, the
        pool's part (``pool_state_dict(stack=False)``: the seed, the act-call counter -- RANDOM's, and the counter of the sampled and
        explored actions too --, the draw counters and the CNN slots' weights as the device holds them).  The env's state is the
        env's (``env.state_dict()``).  With ``pool``, ``load_state_dict`` continues RANDOM's, the sampled and the explored actions
        where the original run's would; a dict WITHOUT it (one saved before the key existed) loads as it always did: that counter
        starts over, and a pool with RANDOM, or with an agent that samples or explores, continues with other such actions than
        the original run."""
        return {"agent_names": list(self.agent_names), "books": self.books.state_dict(), "pairs": self._pairs.cpu().numpy(),
                "stack": self.get_stack().cpu().numpy(), "obs": None if self._buf is None else self._buf.cpu().numpy(), "redraw_on_done": self.redraw_on_done,
                "sampling": np.array([self.sampling()[n] for n in self.agent_names], np.float32).reshape(-1, 2),
                "pool": self.pool_state_dict(stack=False)}

    def load_state_dict(self, sd):
        if list(sd["agent_names"]) != self.agent_names:
            raise ValueError(f"load_state_dict: a pool of {list(sd['agent_names'])} into one of {self.agent_names}")
        # everything is looked at before anything is written: a refused load leaves the arena as it was
        books, p, stack, obs = sd["books"], np.asarray(sd["pairs"]), np.asarray(sd["stack"]), sd.get("obs")
        self.books.check_state_dict(books)
        if p.shape != (self.num_envs, 2) or p.min() < 0 or p.max() >= len(self.agent_names):
            raise ValueError(f"load_state_dict: pairs must be ({self.num_envs}, 2) ids that index agent_names")
        if stack.shape != (2 * self.num_envs, 4, 42, 42):
            raise ValueError(f"load_state_dict: frame rings of shape {stack.shape}, this arena's are {(2 * self.num_envs, 4, 42, 42)}")
        if obs is not None and tuple(np.shape(obs)) != tuple(self.env._obs_shape):
            raise ValueError(f"load_state_dict: an observation buffer of shape {tuple(np.shape(obs))} into an env of {self.env._obs_shape}")
        styles = None  # (a state dict from before the play styles leaves them as they are)
        if sd.get("sampling") is not None:
            styles = np.asarray(sd["sampling"], np.float32)
            if styles.shape != (len(self.agent_names), 2):
                raise ValueError(f"load_state_dict: sampling must hold a (temperature, epsilon) row per agent, got shape {styles.shape}")
            for t, e in styles:
                check_sampling(t, e)
        pool = sd.get("pool")  # (a state dict from before the pool's part: the act-call counter starts over, the slots keep their weights)
        if pool is not None:
            self.check_pool_state_dict(pool)
        self._seed = int(books["seed"])
        if pool is not None:
            self.load_pool_state_dict(pool, styles=False)  # (the styles are the `sampling` key's, below, as before)
        else:
            self._seed_pool(self._seed)
        if styles is not None:
            for a, (t, e) in enumerate(styles):
                self.set_sampling(a, float(t), float(e))
        self.books.load_state_dict(books)
        self.set_pairs(p[:, 0], p[:, 1])
        self.set_stack(np.ascontiguousarray(stack, np.uint8))  # (synchronises)
        if obs is not None:  # (a copy of the arena's own: the env's buffers are drawn again by its next step)
            self._buf = torch.from_numpy(np.ascontiguousarray(obs, np.uint8)).to(self.device)
        self.redraw_on_done = bool(sd["redraw_on_done"])

    def close(self):
        if self._close_pool():
            self.books.close()
            self.env.close()


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
