"""LeagueLedger: how the learner fares against every opponent of a league, kept on the device, and opponent draws weighted by it.

``LeagueEnvWrapper`` gives every env its own opponent; a league trainer also wants per-opponent results (episodes, wins, losses, draws,
summed returns and lengths) and the standard use of them: drawing the next opponent by win rate (prioritised fictitious self-play,
PFSP -- harder opponents more often).  The reference has neither (its ``TournamentEnvWrapper``, pong/competitive_pong_env.py:27-33,
draws ``random.choice(agent_names)``); a trainer on top of it keeps such books on the host.  Here ``update`` is one launch per step with
one lane per env, the weights are made by a one-wavefront kernel from counters that live on the device, and nothing synchronises with the
host unless the caller asks for host values (``counters()``, ``weights()``, ``state_dict()``).

The draw rule and the PFSP rule are written down in include/crl.h ("ledger draws", "PFSP weights") and restated in numpy at the end of
this module (``ledger_draw_reference``, ``pfsp_weights_reference``).  The kernels are HIP behind ``crl_ledger_*`` (csrc/pong_ledger.hip);
there is no torch or CPU path.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N
from .league import league_draw_reference

_MODES = {"hard": N.CRL_LEDGER_PFSP_HARD, "variance": N.CRL_LEDGER_PFSP_VARIANCE}
_A = N.CRL_LEAGUE_MAX_AGENTS


class LeagueLedger:
    """Per-opponent results of ``num_envs`` envs over a pool of ``agents`` agents.  ``env_id_base``: the global id of env 0 (a shard
    passes its own, so that its draws are those of the whole batch); ``seed``: the key of the weighted draws."""

    def __init__(self, num_envs, agents, device, seed=0, env_id_base=0):
        self.num_envs, self.agents = int(num_envs), int(agents)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("LeagueLedger lives on the GPU (there is no CPU fallback)")
        if not 1 <= self.agents <= _A:
            raise ValueError(f"a league holds 1 to {_A} agents, not {agents}")
        self.env_id_base = int(env_id_base)
        self._seed = int(seed) & (2 ** 64 - 1)
        self._L = N.load()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._L.crl_ledger_create(self.device.index or 0, self.num_envs, self.env_id_base, self._seed, self.agents, C.byref(h)))
        self._h = h

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _p(t):
        return C.c_void_p(t.data_ptr()) if t is not None else None

    # ---- the step
    def update(self, assign, reward, done, redraw=False, out=None):
        """One step of the books.  ``assign`` int32 (N,): the opponent every env PLAYED this step against (the assignment before any
        redraw); ``reward`` float32 (N,) or (N, k): the learner's step reward is column 0 (the env's own reward buffer can be passed as
        it is); ``done`` uint8 (N,).  Returns int32 (N,) ids (``out`` if given; it may be ``assign``): ``assign``, with a fresh weighted
        draw where ``done`` is set and ``redraw`` is true.  Device tensors in, device tensor out, no synchronisation."""
        n = self.num_envs
        if assign.dtype != torch.int32 or reward.dtype != torch.float32 or done.dtype != torch.uint8:
            raise TypeError("update(assign int32, reward float32, done uint8): got %s, %s, %s" % (assign.dtype, reward.dtype, done.dtype))
        if assign.numel() != n or done.numel() != n or reward.shape[0] != n or not assign.is_contiguous() or not done.is_contiguous():
            raise ValueError(f"update: contiguous (N,) assign and done and a reward of N rows, N = {n}")
        if reward.dim() > 2:
            raise ValueError("update: reward must be (N,) or (N, k) with the learner's reward in column 0")
        stride = reward.stride(0) if n > 1 else 1
        if out is None:
            out = torch.empty((n,), dtype=torch.int32, device=self.device)
        N.check(self._L.crl_ledger_step(self._h, self._p(assign), self._p(reward), stride, self._p(done), int(bool(redraw)), self._p(out),
                                        self._stream()))
        return out

    # ---- results
    def counters_device(self):
        """int64 (6, 16) device tensor, rows in the order of ``_native.CRL_LEDGER_COUNTER_NAMES``, one column per agent: a copy, enqueued
        on the current stream (no synchronisation).  The shape ``pfsp_weights(counters=...)`` takes, e.g. after an all-reduce."""
        out = torch.empty((N.CRL_LEDGER_COUNTERS, _A), dtype=torch.int64, device=self.device)
        N.check(self._L.crl_ledger_get_counters(self._h, self._p(out), None, self._stream()))
        return out

    def counters(self):
        """Host dict: the six int64 arrays (``episodes``, ``wins``, ``losses``, ``draws``, ``return_sum``, ``length_sum``; one entry per
        agent of the pool), ``ignored`` (episodes whose opponent id was outside the pool) and ``win_rate`` = (wins + draws / 2) /
        episodes (nan for an agent never played).  SYNCHRONISES with the device: not for the hot loop."""
        both = torch.empty((N.CRL_LEDGER_COUNTERS * _A + 1,), dtype=torch.int64, device=self.device)
        N.check(self._L.crl_ledger_get_counters(self._h, self._p(both), C.c_void_p(both.data_ptr() + 8 * N.CRL_LEDGER_COUNTERS * _A), self._stream()))
        host = both.cpu().numpy()
        d = {k: host[i * _A:i * _A + self.agents].copy() for i, k in enumerate(N.CRL_LEDGER_COUNTER_NAMES)}
        d["ignored"] = int(host[-1])
        with np.errstate(invalid="ignore", divide="ignore"):
            d["win_rate"] = (d["wins"] + 0.5 * d["draws"]) / d["episodes"]
        return d

    def env_state(self):
        """Device tensors (ret int32, len int32, draw_ctr as int32 bits) of the running episodes: copies, no synchronisation."""
        t = [torch.empty((self.num_envs,), dtype=torch.int32, device=self.device) for _ in range(3)]
        N.check(self._L.crl_ledger_get_env_state(self._h, self._p(t[0]), self._p(t[1]), self._p(t[2]), self._stream()))
        return tuple(t)

    # ---- weights
    def set_agents(self, agents):
        """The pool grew (``LeagueEnvWrapper.add_agent``): new agents enter the table with weight 1, their counters start at zero."""
        N.check(self._L.crl_ledger_set_agents(self._h, int(agents), self._stream()))
        self.agents = int(agents)

    def set_weights(self, weights):
        """``weights``: one non-negative integer per agent (host values); their sum must lie in [1, 2^32).  Weight 0: never drawn."""
        w = np.asarray(weights)
        if w.shape != (self.agents,) or (w < 0).any() or (w > 0xFFFFFFFF).any():
            raise ValueError(f"set_weights: {self.agents} integers in [0, 2^32)")
        w = np.ascontiguousarray(w, np.uint32)
        N.check(self._L.crl_ledger_set_weights(self._h, w.ctypes.data_as(C.c_void_p), self.agents, self._stream()))

    def pfsp_weights(self, mode="hard", exponent=2, floor=1, counters=None):
        """Fills the table on the device: p = (wins + draws / 2 + 1) / (episodes + 2); ``"hard"``: (1 - p) ** exponent,
        ``"variance"``: p (1 - p); weight = floor + int(f * 65535).  ``counters``: an int64 (6, 16) device tensor in place of the
        ledger's own (a sharded caller passes the all-reduced ``counters_device()`` so that every rank holds the same table).  No
        synchronisation."""
        if mode not in _MODES:
            raise ValueError(f"pfsp_weights: mode must be one of {sorted(_MODES)}")
        if counters is not None:
            if counters.dtype != torch.int64 or tuple(counters.shape) != (N.CRL_LEDGER_COUNTERS, _A) or not counters.is_contiguous() \
                    or counters.device != self.device:
                raise ValueError(f"pfsp_weights: counters must be a contiguous int64 ({N.CRL_LEDGER_COUNTERS}, {_A}) tensor on {self.device}")
        N.check(self._L.crl_ledger_pfsp_weights(self._h, self._p(counters), _MODES[mode], int(exponent), int(floor), self._stream()))

    def weights_device(self):
        """int64 (16,) device tensor holding the uint32 table (entries beyond the pool are 0): a copy, no synchronisation."""
        raw = torch.empty((_A,), dtype=torch.int32, device=self.device)
        N.check(self._L.crl_ledger_get_weights(self._h, self._p(raw), self._stream()))
        return raw.to(torch.int64) & 0xFFFFFFFF

    def weights(self):
        """The table of the pool's agents as a host uint32 array (synchronises)."""
        return self.weights_device()[:self.agents].cpu().numpy().astype(np.uint32)

    # ---- lifetime
    def seed(self, s):
        """New key for the draws; every env's draw counter starts over.  Results and weights stay."""
        self._seed = int(s or 0) & (2 ** 64 - 1)
        N.check(self._L.crl_ledger_seed(self._h, self._seed, self._stream()))

    def reset(self):
        """Zeroes the counters and the running returns / lengths (weights, key and draw counters stay)."""
        N.check(self._L.crl_ledger_reset(self._h, self._stream()))

    def state_dict(self):
        """Everything a continuation needs, as host arrays (synchronises)."""
        both = torch.empty((N.CRL_LEDGER_COUNTERS * _A + 1,), dtype=torch.int64, device=self.device)
        N.check(self._L.crl_ledger_get_counters(self._h, self._p(both), C.c_void_p(both.data_ptr() + 8 * N.CRL_LEDGER_COUNTERS * _A), self._stream()))
        ret, length, ctr = self.env_state()
        return {"agents": self.agents, "seed": self._seed, "counters": both[:-1].reshape(N.CRL_LEDGER_COUNTERS, _A).cpu().numpy(),
                "ignored": int(both[-1].cpu()), "ret": ret.cpu().numpy(), "len": length.cpu().numpy(),
                "draw_ctr": ctr.cpu().numpy().view(np.uint32), "weights": self.weights()}

    def load_state_dict(self, sd):
        if int(sd["agents"]) != self.agents or len(sd["ret"]) != self.num_envs:
            raise ValueError(f"load_state_dict: a ledger of {sd['agents']} agents x {len(sd['ret'])} envs into one of {self.agents} x {self.num_envs}")
        self.seed(sd["seed"])  # (zeroes the draw counters; they are written below)
        both = torch.from_numpy(np.concatenate([np.asarray(sd["counters"], np.int64).reshape(-1), [np.int64(sd["ignored"])]])).to(self.device)
        N.check(self._L.crl_ledger_set_counters(self._h, self._p(both), C.c_void_p(both.data_ptr() + 8 * N.CRL_LEDGER_COUNTERS * _A), self._stream()))
        t = [torch.from_numpy(np.ascontiguousarray(sd[k]).view(np.int32).copy()).to(self.device) for k in ("ret", "len", "draw_ctr")]
        N.check(self._L.crl_ledger_set_env_state(self._h, self._p(t[0]), self._p(t[1]), self._p(t[2]), self._stream()))
        self.set_weights(sd["weights"])
        torch.cuda.current_stream(self.device).synchronize()  # the staging tensors above are this call's own

    def close(self):
        if getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            self._L.crl_ledger_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._L.crl_ledger_destroy(self._h)
                self._h = None
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass


def ledger_draw_reference(seed, gid, counter, weights):
    """The ledger's weighted draw in numpy (include/crl.h "ledger draws"): x = Philox4x32-10 word 0 of counter (gid lo, gid hi, counter,
    CRL_LEDGER_DOMAIN_OPPONENT) under the seed; r = (x * T) >> 32 with T the sum of the weights; the smallest agent whose cumulative
    weight exceeds r.  Arrays broadcast; returns int64.  Host code for tests and for callers that want to predict a draw; the
    kernels do not use it."""
    w = np.asarray(weights)
    if w.ndim != 1 or not 1 <= len(w) <= _A or (w < 0).any():
        raise ValueError(f"1 to {_A} non-negative weights")
    total = int(w.astype(np.uint64).sum())
    if not 0 < total < 2 ** 32:
        raise ValueError(f"the weights must sum to a value in [1, 2^32), not {total}")
    r = league_draw_reference(seed, gid, counter, N.CRL_LEDGER_DOMAIN_OPPONENT, total)  # (x * T) >> 32
    return np.searchsorted(np.cumsum(w.astype(np.int64)), r, side="right").astype(np.int64)


def pfsp_weights_reference(counters, agents, mode="hard", exponent=2, floor=1):
    """The PFSP weight table in numpy (include/crl.h "PFSP weights"), bit for bit what the device kernel writes: float64 with one
    rounding per operation.  ``counters``: int64 (6, 16) in the order of ``_native.CRL_LEDGER_COUNTER_NAMES``.  Returns uint32 (16,);
    entries beyond ``agents`` are 0."""
    c = np.asarray(counters, np.int64).reshape(N.CRL_LEDGER_COUNTERS, _A)
    if mode not in _MODES or (mode == "hard" and int(exponent) < 1):
        raise ValueError("mode 'hard' (exponent >= 1) or 'variance'")
    episodes, wins, draws = (c[i].astype(np.float64) for i in (0, 1, 3))
    p = ((wins + np.float64(0.5) * draws) + np.float64(1.0)) / (episodes + np.float64(2.0))
    q = np.float64(1.0) - p
    if mode == "variance":
        f = p * q
    else:
        f = q.copy()
        for _ in range(int(exponent) - 1):
            f = f * q
    w = (np.int64(floor) + np.floor(f * np.float64(65535.0)).astype(np.int64)).astype(np.uint32)
    w[int(agents):] = 0
    return w
