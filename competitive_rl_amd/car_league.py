"""CarLeague: per-env opponents for car 1 of a two-car CarRacing env and the books of every race, on the device (include/crl.h "car
league") -- for CarRacing what ``LeagueEnvWrapper`` with a ``LeagueLedger`` is for Pong.

The env resets a finished episode inside ``step_device``; a trainer that wants "a fresh opponent per episode, harder ones more often"
would otherwise read ``done`` on the host, draw with torch and push two assignment tensors.  Here ``step`` is one launch per env step
with one lane per env: it sums both cars' rewards, books a finished episode under the pool entry that drove car 1 (episodes, wins,
losses, draws, both return sums in units of 1/256, length sum -- 64-bit integers, so the totals do not depend on arrival order), draws
the env's next opponent by the weight table and writes it into column 1 of the policy's and the drivers' own device assignment arrays.
The next ``drivers.act`` / ``policy.act`` on the stream serves it from the first step of the new episode.  Car 0 is the caller's:
column 0 is never touched.  Nothing synchronises with the host unless the caller asks for host values.

    env = HipCarVecEnv(n, done_policy="car0")
    policy, drivers = CarPolicy(env), CarDrivers(env)
    policy.add_network("learner", w), policy.add_network("snapshot", w)
    policy.assign(0, "learner")
    league = CarLeague(env, policy, drivers, seed=0)
    league.add_style("RANDOM"), league.add_style("RULE_BASED"), league.add_network("snapshot")
    env.reset()
    league.reset_assignment()
    for _ in range(steps):
        drivers.act(actions), policy.act(actions)
        _, rewards, done = env.step_device(actions, render=False)
        league.step(rewards, done)
    league.pfsp_weights("hard", 2, 1)
    print(league.counters()["win_rate"])

The rule is restated in numpy by ``rules.car_league_reference`` and ``rules.car_league_draw_reference``; the kernels are HIP behind
``crl_car_league_*`` (csrc/car_league.hip); there is no torch or CPU path.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N
from . import checkpoint as ck
from .books import WeightTable, _p
from .rules import CAR_LEAGUE_KINDS

__all__ = ["CarLeague"]

_A = N.CRL_LEAGUE_MAX_AGENTS
_NAMES = N.CRL_CAR_LEAGUE_COUNTER_NAMES


class CarLeague(WeightTable):
    """A pool of up to 16 opponents for car 1 of ``env`` -- networks of ``policy`` and styles of ``drivers`` -- with per-env draws and
    per-agent books.  ``seed``: the key of the draws; the env's ``env_id_base`` makes a shard draw what the whole batch would.  The
    weight table (``set_weights``, ``weights_device``, ``weights``), ``seed`` and ``reset`` are ``books.WeightTable``'s."""

    _C, _COUNTERS = "crl_car_league_", (len(_NAMES), _A)

    def __init__(self, env, policy, drivers, seed=0):
        env = getattr(env, "env", env)  # (a HipCompetitiveCarVecEnv wraps its HipCarVecEnv)
        if not hasattr(env, "_h") or not hasattr(env, "P"):
            raise TypeError("CarLeague needs a HipCarVecEnv")
        env._check_open(), policy._check_open(), drivers._check_open()
        if policy.env is not env or drivers.env is not env:
            raise ValueError("CarLeague: the policy and the drivers must belong to this env")
        self.env, self.policy, self.drivers, self._L = env, policy, drivers, env._L
        self.num_envs, self.device = env.num_envs, env.device
        self._seed = int(seed) & (2 ** 64 - 1)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._L.crl_car_league_create(env._h, policy._h, drivers._h, self._seed, C.byref(h)))
        self._h = h
        self._pool = []  # (kind name, agent name, slot) by agent id

    # ---- plumbing
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check_open(self):
        if self._h is None or self.env.closed or self.policy._h is None or self.drivers._h is None:  # (it writes into both objects' arrays)
            raise RuntimeError("CarLeague (or its env, policy or drivers) is closed")

    def close(self):
        if self._h is not None:
            if not self.env.closed:
                torch.cuda.synchronize(self.device)
            self._L.crl_car_league_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- the pool
    @property
    def agents(self):
        return len(self._pool)

    def agent_names(self):
        return tuple(name for _, name, _ in self._pool)

    def agent_id(self, name):
        names = self.agent_names()
        if name not in names:
            raise ValueError(f"Unknown league agent {name!r}; known: {names}")
        return names.index(name)

    def pool(self):
        """The pool as (kind, slot) per agent id, the form ``rules.car_league_columns`` takes."""
        return [(kind, slot) for kind, _, slot in self._pool]

    def _add(self, kind, name, slot):
        self._check_open()
        if name in self.agent_names():
            raise ValueError(f"{name!r} is in the pool already")
        if len(self._pool) >= _A:
            raise ValueError(f"the pool holds {_A} agents already")
        out = C.c_int32()
        N.check(self._L.crl_car_league_add_agent(self._h, CAR_LEAGUE_KINDS.index(kind), int(slot), C.byref(out), self._stream()))
        self._pool.append((kind, name, int(slot)))
        return out.value

    def add_network(self, name):
        """Network ``name`` of the policy joins the pool (weight 1); returns its agent id."""
        return self._add("NETWORK", name, self.policy.slot_of(name))

    def add_style(self, name):
        """Style ``name`` of the drivers joins the pool (weight 1); returns its agent id."""
        return self._add("STYLE", name, self.drivers.slot_of(name))

    # ---- draws and the step
    def reset_assignment(self):
        """A fresh draw for every env (after ``env.reset()``), written into car 1's column of both assignments.  No synchronisation."""
        self._check_open()
        N.check(self._L.crl_car_league_draw_all(self._h, self._stream()))

    def step(self, rewards, done, redraw=True):
        """One step of the books, behind the ``env.step_device`` that returned ``rewards`` float32 (N, 2) and ``done`` uint8 (N,): sums
        the rewards, books finished episodes under the agent that drove them and, with ``redraw``, gives their envs a fresh weighted
        draw.  One launch on the current stream, no synchronisation."""
        self._check_open()
        n = self.num_envs
        if not (isinstance(rewards, torch.Tensor) and isinstance(done, torch.Tensor)) or rewards.dtype != torch.float32 or done.dtype != torch.uint8:
            raise TypeError("step(rewards float32, done uint8): device tensors of these dtypes")
        if rewards.device != self.device or done.device != self.device:
            raise ValueError(f"step: rewards and done must live on {self.device}")
        if tuple(rewards.shape) != (n, 2) or tuple(done.shape) != (n,) or not rewards.is_contiguous() or not done.is_contiguous():
            raise ValueError(f"step: a contiguous ({n}, 2) rewards and a contiguous ({n},) done")
        N.check(self._L.crl_car_league_step(self._h, _p(rewards), _p(done), int(bool(redraw)), self._stream()))

    def assignment(self):
        """The agent id that drives car 1 of every env: int32 (N,) on the device (a copy, no synchronisation); -1 before a draw."""
        self._check_open()
        out = torch.empty((self.num_envs,), dtype=torch.int32, device=self.device)
        N.check(self._L.crl_car_league_get_assignment(self._h, _p(out), self._stream()))
        return out

    # ---- results
    def counters_device(self):
        """int64 (7, 16) device tensor, one plane per counter in the order of ``_native.CRL_CAR_LEAGUE_COUNTER_NAMES``: a copy on the
        current stream, no synchronisation.  The shape ``pfsp_weights(counters=...)`` takes, e.g. after an all-reduce."""
        self._check_open()
        out = torch.empty((len(_NAMES), _A), dtype=torch.int64, device=self.device)
        N.check(self._L.crl_car_league_get_counters(self._h, _p(out), self._stream()))
        return out

    def counters(self):
        """Host dict: the seven int64 arrays, one entry per agent of the pool, plus ``win_rate`` = (wins + draws / 2) / episodes and
        ``mean_return`` / ``mean_opponent_return`` in reward units (sum / 256 / episodes); nan for an agent never played.
        SYNCHRONISES with the device: not for the hot loop."""
        planes = self.counters_device().cpu().numpy()
        d = {k: planes[i, :self.agents].copy() for i, k in enumerate(_NAMES)}
        with np.errstate(invalid="ignore", divide="ignore"):
            d["win_rate"] = (d["wins"] + 0.5 * d["draws"]) / d["episodes"]
            d["mean_return"] = d["return_sum"] / 256.0 / d["episodes"]
            d["mean_opponent_return"] = d["opponent_return_sum"] / 256.0 / d["episodes"]
        return d

    def env_state(self):
        """Device tensors (agent int32 (N,), ret float32 (N, 2), len int32 (N,), draw_ctr as int32 bits (N,)): copies, no
        synchronisation."""
        self._check_open()
        n, dev = self.num_envs, self.device
        agent, length, ctr = (torch.empty((n,), dtype=torch.int32, device=dev) for _ in range(3))
        ret = torch.empty((n, 2), dtype=torch.float32, device=dev)
        N.check(self._L.crl_car_league_get_env_state(self._h, _p(agent), _p(ret), _p(length), _p(ctr), self._stream()))
        return agent, ret, length, ctr

    # ---- weights
    def pfsp_weights(self, mode="hard", exponent=2, floor=1, counters=None):
        """Fills the table on the device by the rule of ``LeagueLedger.pfsp_weights`` over this league's episodes, wins and draws:
        agents car 0 loses to are drawn more often.  ``counters``: an int64 (7, 16) device tensor in place of the league's own (a
        sharded caller passes the all-reduced ``counters_device()``).  No synchronisation."""
        self._pfsp_weights(mode, exponent, floor, counters)

    # ---- lifetime
    def reset_agent(self, name):
        """Zeroes the counters of agent ``name``: its slot took a newer snapshot, the record starts over."""
        self._check_open()
        N.check(self._L.crl_car_league_reset_agent(self._h, self.agent_id(name), self._stream()))

    # ---- checkpoint / resume
    def state_dict(self):
        """Everything a continuation needs, as host arrays and scalars (synchronises)."""
        self._check_open()
        counters = self.counters_device().cpu().numpy()
        agent, ret, length, ctr = (t.cpu().numpy() for t in self.env_state())
        return {"kind": "CarLeague", "num_envs": self.num_envs, "seed": self._seed,
                "pool": [dict(kind=kind, name=name, slot=slot) for kind, name, slot in self._pool], "counters": counters,
                "agent": agent, "ret": ret, "len": length, "draw_ctr": ctr.view(np.uint32), "weights": self.weights()}

    def load_state_dict(self, sd):
        """Pool, books, per-env state, key and weights of a ``state_dict()``.  The saved pool must continue this object's (a fresh
        league's is empty) and name networks and styles that ``policy`` and ``drivers`` hold in the same slots -- load theirs first.
        Everything is looked at before anything is written: a refused load raises ``ValueError`` and leaves the object as it was."""
        self._check_open()
        what = "CarLeague"
        ck.check_header(sd, "CarLeague", what, num_envs=self.num_envs)
        seed = ck.check_counter(sd.get("seed"), 64, "seed", what)
        pool = sd.get("pool")
        if not isinstance(pool, (list, tuple)) or not len(self._pool) <= len(pool) <= _A:
            raise ck.refuse(f"{what}: pool must be a list of {len(self._pool)} to {_A} entries")
        parsed = []
        for a, entry in enumerate(pool):
            try:
                kind, name, slot = entry["kind"], entry["name"], int(entry["slot"])
            except (KeyError, TypeError, ValueError) as e:
                raise ck.refuse(f"{what}: pool entry {a}: {e!r}") from None
            if kind not in CAR_LEAGUE_KINDS or not isinstance(name, str):
                raise ck.refuse(f"{what}: pool entry {a}: kind must be one of {CAR_LEAGUE_KINDS} and name a string")
            holder = self.policy if kind == "NETWORK" else self.drivers
            if holder._slots.get(name) != slot:
                raise ck.refuse(f"{what}: pool entry {a}: {kind.lower()} {name!r} in slot {slot} is not what the {type(holder).__name__} holds")
            if a < len(self._pool) and self._pool[a] != (kind, name, slot):
                raise ck.refuse(f"{what}: pool entry {a} is {self._pool[a]} here")
            parsed.append((kind, name, slot))
        if len({name for _, name, _ in parsed}) != len(parsed):
            raise ck.refuse(f"{what}: the pool names an agent twice")
        counters = ck.check_array(sd, "counters", (len(_NAMES), _A), 8, what).view(np.int64)
        n = self.num_envs
        agent = ck.check_array(sd, "agent", (n,), 4, what).view(np.int32)
        ret = ck.check_array(sd, "ret", (n, 2), 4, what).view(np.float32)
        length = ck.check_array(sd, "len", (n,), 4, what).view(np.int32)
        ctr = ck.check_array(sd, "draw_ctr", (n,), 4, what).view(np.int32)
        if ((agent < -1) | (agent >= len(parsed))).any():
            raise ck.refuse(f"{what}: agent holds ids outside [-1, {len(parsed)})")
        w = np.asarray(sd.get("weights"))
        if w.shape != (len(parsed),) or w.dtype.kind not in "iu" or (w < 0).any() or (w > 0xFFFFFFFF).any():
            raise ck.refuse(f"{what}: weights must be {len(parsed)} integers in [0, 2^32)")
        w = np.ascontiguousarray(w, np.uint32)
        if len(parsed) and not 0 < int(w.sum(dtype=np.uint64)) < 2 ** 32:
            raise ck.refuse(f"{what}: the weights must sum to a value in [1, 2^32)")
        for kind, name, slot in parsed[len(self._pool):]:
            self._add(kind, name, slot)
        self.seed(seed)
        dev = [torch.from_numpy(a.copy()).to(self.device) for a in (counters, agent, ret, length, ctr)]
        N.check(self._L.crl_car_league_set_counters(self._h, _p(dev[0]), self._stream()))
        N.check(self._L.crl_car_league_set_env_state(self._h, _p(dev[1]), _p(dev[2]), _p(dev[3]), _p(dev[4]), self._stream()))
        if len(parsed):
            self.set_weights(w)
        torch.cuda.current_stream(self.device).synchronize()  # the staging tensors above are this call's own
