"""DeviceBooks: what ``LeagueLedger`` (ledger.py) and ``ArenaBooks`` (arena.py) share -- the same device object with another key
(csrc/pong_books.h): an opponent's id in the ledger, a (left, right) cell in the arena.  A subclass names its C prefix, its counters and
the shape of one counter plane; its weight table is that plane cut to the pool.  The handle, the checks of ``update``, the copies of
counters and per-env state, ``state_dict`` / ``load_state_dict`` and the lifetime live here.

``WeightTable`` is the part that ``CarLeague`` (car_league.py) shares as well, an object with per-env state of its own: the weight
table of a pool behind a C prefix -- its check, ``set_weights`` / ``weights_device`` / ``weights``, ``seed`` / ``reset`` and the checks
of a PFSP fill.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N

_A = N.CRL_LEAGUE_MAX_AGENTS


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


PFSP_MODES = {"hard": N.CRL_LEDGER_PFSP_HARD, "variance": N.CRL_LEDGER_PFSP_VARIANCE}


class WeightTable:
    """The weight table of a pool of ``self.agents`` agents behind ``self._C`` + set_weights / get_weights / seed / reset (and
    pfsp_weights where the table holds one weight per agent).  The host object has ``_L``, ``_h``, ``device``, ``_stream()``, the shape
    ``_PLANE`` of the device's table and the shape ``_COUNTERS`` of its counter planes."""

    _C = None
    _PLANE = (_A,)
    _COUNTERS = ()

    def _c(self, name):
        return getattr(self._L, self._C + name)

    def _check_open(self):
        """Raises where a call would write into something closed (``CarLeague``); the Pong books have no such check."""

    def _weight_table(self, weights, what):
        w = np.asarray(weights)
        shape = (self.agents,) * len(self._PLANE)
        if w.shape != shape or not w.size or (w < 0).any() or (w > 0xFFFFFFFF).any():
            raise ValueError(f"{what}: {shape} integers in [0, 2^32)")
        return np.ascontiguousarray(w, np.uint32)

    def set_weights(self, weights):
        """``weights``: one non-negative integer per agent / per [left][right] cell of the pool (host values); their sum must lie in
        [1, 2^32).  Weight 0: never drawn."""
        self._check_open()
        w = self._weight_table(weights, "set_weights")
        N.check(self._c("set_weights")(self._h, w.ctypes.data_as(C.c_void_p), w.size, self._stream()))

    def weights_device(self):
        """int64 device tensor of the shape of a counter plane holding the uint32 table (entries beyond the pool are 0): a copy, no
        synchronisation."""
        self._check_open()
        raw = torch.empty(self._PLANE, dtype=torch.int32, device=self.device)
        N.check(self._c("get_weights")(self._h, _p(raw), self._stream()))
        return raw.to(torch.int64) & 0xFFFFFFFF

    def weights(self):
        """The table of the pool as a host uint32 array (synchronises)."""
        return self.weights_device()[(slice(0, self.agents),) * len(self._PLANE)].cpu().numpy().astype(np.uint32)

    def _check_counters(self, counters, what):
        if counters is not None and (not isinstance(counters, torch.Tensor) or counters.dtype != torch.int64 or tuple(counters.shape) != self._COUNTERS
                                     or not counters.is_contiguous() or counters.device != self.device):
            raise ValueError(f"{what}: counters must be a contiguous int64 {self._COUNTERS} tensor on {self.device}")

    def _pfsp_weights(self, mode, exponent, floor, counters):
        """``pfsp_weights`` of a table of one weight per agent, behind the checks of ``mode`` and ``counters``."""
        self._check_open()
        if mode not in PFSP_MODES:
            raise ValueError(f"pfsp_weights: mode must be one of {sorted(PFSP_MODES)}")
        self._check_counters(counters, "pfsp_weights")
        N.check(self._c("pfsp_weights")(self._h, _p(counters), PFSP_MODES[mode], int(exponent), int(floor), self._stream()))

    def seed(self, seed):
        """New key for the draws; every env's draw counter starts over.  Results, weights and what the envs hold stay."""
        self._check_open()
        self._seed = int(seed or 0) & (2 ** 64 - 1)
        N.check(self._c("seed")(self._h, self._seed, self._stream()))

    def reset(self):
        """Zeroes the counters and the running returns / lengths (weights, key, draw counters and assignments stay)."""
        self._check_open()
        N.check(self._c("reset")(self._h, self._stream()))


class DeviceBooks(WeightTable):
    """Results of ``num_envs`` envs over a pool of ``agents`` agents and the weighted draw of an env's next ids.  ``env_id_base``: the
    global id of env 0 (a shard passes its own, so that its draws are those of the whole batch); ``seed``: the key of the draws."""

    _C = None      # "crl_ledger_" / "crl_arena_"
    _NAMES = ()    # the counter planes, in the library's order
    _PLANE = ()    # shape of one counter plane: (16,) / (16, 16)

    def __init__(self, num_envs, agents, device, seed=0, env_id_base=0):
        self.num_envs, self.agents = int(num_envs), int(agents)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} lives on the GPU (there is no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        if not 1 <= self.agents <= _A:
            raise ValueError(f"a pool holds 1 to {_A} agents, not {agents}")
        self.env_id_base = int(env_id_base)
        self._seed = int(seed) & (2 ** 64 - 1)
        self._L = N.load()
        self._COUNTERS = (len(self._NAMES),) + self._PLANE
        self._words = int(np.prod(self._COUNTERS))  # int64 counter words; `ignored` follows them
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._c("create")(self.device.index, self.num_envs, self.env_id_base, self._seed, self.agents, C.byref(h)))
        self._h = h

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _pool(self):
        """The index that cuts a plane to the pool."""
        return (slice(0, self.agents),) * len(self._PLANE)

    # ---- the step
    def _step(self, ids, reward, done, redraw, out):
        """``crl_*_step`` behind the checks that do not depend on the key; ``ids`` and ``out`` were checked by the subclass."""
        n = self.num_envs
        if reward.dtype != torch.float32 or done.dtype != torch.uint8:
            raise TypeError("update(ids int32, reward float32, done uint8): got %s, %s, %s" % (ids.dtype, reward.dtype, done.dtype))
        if done.numel() != n or reward.shape[0] != n or not done.is_contiguous() or reward.dim() > 2:
            raise ValueError(f"update: a contiguous (N,) done and a reward of N rows, (N,) or (N, k) with column 0 the one booked, N = {n}")
        stride = reward.stride(0) if n > 1 else 1
        N.check(self._c("step")(self._h, _p(ids), _p(reward), stride, _p(done), int(bool(redraw)), _p(out), self._stream()))
        return out

    # ---- results
    def _counters_and_ignored(self):
        both = torch.empty((self._words + 1,), dtype=torch.int64, device=self.device)
        N.check(self._c("get_counters")(self._h, _p(both), C.c_void_p(both.data_ptr() + 8 * self._words), self._stream()))
        return both

    def counters_device(self):
        """int64 device tensor of one plane per counter (``_NAMES`` order): a copy, enqueued on the current stream (no synchronisation).
        The shape the subclass's weight rule takes as ``counters=...``, e.g. after an all-reduce."""
        out = torch.empty((len(self._NAMES),) + self._PLANE, dtype=torch.int64, device=self.device)
        N.check(self._c("get_counters")(self._h, _p(out), None, self._stream()))
        return out

    def counters(self):
        """Host dict: one int64 array per counter, cut to the pool, and ``ignored`` (episodes with an id outside the pool).
        SYNCHRONISES with the device: not for the hot loop."""
        host = self._counters_and_ignored().cpu().numpy()
        planes = host[:-1].reshape((len(self._NAMES),) + self._PLANE)
        d = {k: planes[i][self._pool()].copy() for i, k in enumerate(self._NAMES)}
        d["ignored"] = int(host[-1])
        return d

    def env_state(self):
        """Device tensors (ret int32, len int32, draw_ctr as int32 bits) of the running episodes: copies, no synchronisation."""
        t = [torch.empty((self.num_envs,), dtype=torch.int32, device=self.device) for _ in range(3)]
        N.check(self._c("get_env_state")(self._h, _p(t[0]), _p(t[1]), _p(t[2]), self._stream()))
        return tuple(t)

    # ---- weights
    def set_agents(self, agents):
        """The pool grew (``add_agent``): what is new enters the table with weight 1 (the arena's diagonal: 0).  Only the weight table
        changes: the counters are what they were (zero unless the pool held the agent before or ``load_state_dict`` wrote them)."""
        N.check(self._c("set_agents")(self._h, int(agents), self._stream()))
        self.agents = int(agents)

    # ---- lifetime (the table, ``seed`` and ``reset`` are ``WeightTable``'s)
    def state_dict(self):
        """Everything a continuation needs, as host arrays (synchronises)."""
        both = self._counters_and_ignored().cpu().numpy()
        ret, length, ctr = self.env_state()
        return {"agents": self.agents, "seed": self._seed, "counters": both[:-1].reshape((len(self._NAMES),) + self._PLANE).copy(),
                "ignored": int(both[-1]), "ret": ret.cpu().numpy(), "len": length.cpu().numpy(),
                "draw_ctr": ctr.cpu().numpy().view(np.uint32), "weights": self.weights()}

    def check_state_dict(self, sd):
        """What ``load_state_dict`` refuses, raised before anything is written.  Returns (counters, weights, (ret, len, draw_ctr))."""
        if int(sd["agents"]) != self.agents or len(sd["ret"]) != self.num_envs:
            raise ValueError(f"load_state_dict: books of {sd['agents']} agents x {len(sd['ret'])} envs into ones of {self.agents} x {self.num_envs}")
        counters = np.asarray(sd["counters"], np.int64)
        if counters.size != self._words:
            raise ValueError(f"load_state_dict: counters of {(len(self._NAMES),) + self._PLANE} are needed, not of {counters.shape}")
        w = self._weight_table(sd["weights"], "load_state_dict: weights")
        if int(w.sum(dtype=np.uint64)) >= 2 ** 32:
            raise ValueError("load_state_dict: the weights must sum to a value below 2^32")
        if not w.any() and self.weights().any():
            raise ValueError(f"load_state_dict: an all-zero weight table cannot be set ({self._C}set_weights refuses a sum of 0)")
        env = [np.ascontiguousarray(sd[k]) for k in ("ret", "len", "draw_ctr")]
        if any(a.shape != (self.num_envs,) or a.dtype.itemsize != 4 for a in env):
            raise ValueError(f"load_state_dict: ret, len and draw_ctr must be 32-bit arrays of {self.num_envs} envs")
        return counters, w, env

    def load_state_dict(self, sd):
        """Everything is looked at before anything is written: a refused load leaves the books as they were."""
        counters, w, env = self.check_state_dict(sd)
        self.seed(sd["seed"])  # (zeroes the draw counters; they are written below)
        both = torch.from_numpy(np.concatenate([counters.reshape(-1), [np.int64(sd["ignored"])]])).to(self.device)
        N.check(self._c("set_counters")(self._h, _p(both), C.c_void_p(both.data_ptr() + 8 * self._words), self._stream()))
        t = [torch.from_numpy(a.view(np.int32).copy()).to(self.device) for a in env]
        N.check(self._c("set_env_state")(self._h, _p(t[0]), _p(t[1]), _p(t[2]), self._stream()))
        if w.any():  # (an all-zero table is the one in force already)
            self.set_weights(w)
        torch.cuda.current_stream(self.device).synchronize()  # the staging tensors above are this call's own

    def close(self):
        if getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            self._c("destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                self._c("destroy")(self._h)
                self._h = None
        except Exception:  # noqa: BLE001  (interpreter shutdown)
            pass
