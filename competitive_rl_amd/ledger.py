"""LeagueLedger: how the learner fares against every opponent of a league, kept on the device, and opponent draws weighted by it.

``LeagueEnvWrapper`` gives every env its own opponent; a league trainer also wants per-opponent results (episodes, wins, losses, draws,
summed returns and lengths) and the standard use of them: drawing the next opponent by win rate (prioritised fictitious self-play,
PFSP -- harder opponents more often).  The reference has neither (its ``TournamentEnvWrapper``, pong/competitive_pong_env.py:27-33,
draws ``random.choice(agent_names)``); a trainer on top of it keeps such books on the host.  Here ``update`` is one launch per step with
one lane per env, the weights are made by a one-wavefront kernel from counters that live on the device, and nothing synchronises with the
host unless the caller asks for host values (``counters()``, ``weights()``, ``state_dict()``).

The draw rule and the PFSP rule are written down in include/crl.h ("ledger draws", "PFSP weights") and restated in numpy at the end of
this module (``ledger_draw_reference``, ``pfsp_weights_reference``).  The kernels are HIP behind ``crl_ledger_*`` (csrc/pong_ledger.hip
over the core it shares with the arena's books, csrc/pong_books.h; here ``DeviceBooks`` of books.py is that shared part); there is no
torch or CPU path.
"""
import numpy as np
import torch

from . import _native as N
from .books import PFSP_MODES as _MODES
from .books import DeviceBooks
from .rules import weighted_draw_reference

_A = N.CRL_LEAGUE_MAX_AGENTS


class LeagueLedger(DeviceBooks):
    """Per-opponent results of ``num_envs`` envs over a pool of ``agents`` agents (``DeviceBooks`` keyed by the opponent's id): counter
    planes int64 (6, 16) in the order of ``_native.CRL_LEDGER_COUNTER_NAMES``, one column per agent; one weight per agent."""

    _C, _NAMES, _PLANE = "crl_ledger_", N.CRL_LEDGER_COUNTER_NAMES, (_A,)

    def update(self, assign, reward, done, redraw=False, out=None):
        """One step of the books.  ``assign`` int32 (N,): the opponent every env PLAYED this step against (the assignment before any
        redraw); ``reward`` float32 (N,) or (N, k): the learner's step reward is column 0 (the env's own reward buffer can be passed as
        it is); ``done`` uint8 (N,).  Returns int32 (N,) ids (``out`` if given; it may be ``assign``): ``assign``, with a fresh weighted
        draw where ``done`` is set and ``redraw`` is true.  Device tensors in, device tensor out, no synchronisation."""
        if assign.dtype != torch.int32:
            raise TypeError("update(assign int32, reward float32, done uint8): got %s, %s, %s" % (assign.dtype, reward.dtype, done.dtype))
        if assign.numel() != self.num_envs or not assign.is_contiguous():
            raise ValueError(f"update: a contiguous (N,) assign, N = {self.num_envs}")
        if out is None:
            out = torch.empty((self.num_envs,), dtype=torch.int32, device=self.device)
        return self._step(assign, reward, done, redraw, out)

    def counters(self):
        """Host dict: the six int64 arrays (``episodes``, ``wins``, ``losses``, ``draws``, ``return_sum``, ``length_sum``; one entry per
        agent of the pool), ``ignored`` (episodes whose opponent id was outside the pool) and ``win_rate`` = (wins + draws / 2) /
        episodes (nan for an agent never played).  SYNCHRONISES with the device: not for the hot loop."""
        d = super().counters()
        with np.errstate(invalid="ignore", divide="ignore"):
            d["win_rate"] = (d["wins"] + 0.5 * d["draws"]) / d["episodes"]
        return d

    def pfsp_weights(self, mode="hard", exponent=2, floor=1, counters=None):
        """Fills the table on the device: p = (wins + draws / 2 + 1) / (episodes + 2); ``"hard"``: (1 - p) ** exponent,
        ``"variance"``: p (1 - p); weight = floor + int(f * 65535).  ``counters``: an int64 (6, 16) device tensor in place of the
        ledger's own (a sharded caller passes the all-reduced ``counters_device()`` so that every rank holds the same table).  No
        synchronisation."""
        self._pfsp_weights(mode, exponent, floor, counters)


def ledger_draw_reference(seed, gid, counter, weights):
    """The ledger's weighted draw in numpy (include/crl.h "ledger draws"): x = Philox4x32-10 word 0 of counter (gid lo, gid hi, counter,
    CRL_LEDGER_DOMAIN_OPPONENT) under the seed; r = (x * T) >> 32 with T the sum of the weights; the smallest agent whose cumulative
    weight exceeds r.  Arrays broadcast; returns int64.  Host code for tests and for callers that want to predict a draw; the
    kernels do not use it."""
    w = np.asarray(weights)
    if w.ndim != 1 or not 1 <= len(w) <= _A or (w < 0).any():
        raise ValueError(f"1 to {_A} non-negative weights")
    return weighted_draw_reference(seed, gid, counter, N.CRL_LEDGER_DOMAIN_OPPONENT, w)


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
