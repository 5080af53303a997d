"""Built-in CarRacing agents served on the device (include/crl.h "car drivers"): RANDOM and the track-following RULE_BASED driver,
assignable per env and per car.

The reference's ``make_competitive_car_racing(opponent_policy, ...)`` (car_racing/make_competitive_car_racing.py:10-58) takes a Python
callable and ships no agent to pass; Pong has ``get_builtin_agent_names()`` (pong/builtin_policies.py:14-15).  ``CarDrivers`` is the
CarRacing counterpart: it reads the env's own device state (RULE_BASED reads the state as Pong's cheat code does) and fills the
assigned cars' rows of the action tensor the next ``step_device`` takes -- one launch, no host synchronisation.

    env = HipCarVecEnv(n)
    drivers = CarDrivers(env, seed=0)
    drivers.set_style("careful", target_speed=30.0, epsilon=0.1)
    drivers.assign(0, "RULE_BASED")
    drivers.assign(1, "careful")
    actions = torch.zeros((n, 2, 2), device=env.device)
    env.reset()
    for _ in range(steps):
        drivers.act(actions)
        env.step_device(actions)
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N
from . import checkpoint as ck
from .rules import CAR_DRIVER_KINDS, check_car_style

__all__ = ["CarDrivers", "get_builtin_car_driver_names"]


def get_builtin_car_driver_names():
    """The styles every ``CarDrivers`` starts with (slots 0 and 1), and the names ``make_competitive_car_racing`` accepts."""
    return CAR_DRIVER_KINDS


class CarDrivers:
    def __init__(self, env, seed=0):
        env = getattr(env, "env", env)  # (a HipCompetitiveCarVecEnv wraps its HipCarVecEnv)
        if not hasattr(env, "_h") or not hasattr(env, "P"):
            raise TypeError("CarDrivers needs a HipCarVecEnv")
        env._check_open()
        self.env, self._L = env, env._L
        self.num_envs, self.players, self.device = env.num_envs, env.P, env.device
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._L.crl_car_driver_create(env._h, int(seed) & (2 ** 64 - 1), C.byref(h)))
        self._h = h
        self._slots = {name: k for k, name in enumerate(CAR_DRIVER_KINDS)}  # style name -> slot; RANDOM = 0, RULE_BASED = 1
        self._assign = torch.full((self.num_envs, self.players), -1, dtype=torch.int32, device=self.device)

    # ---- plumbing
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check_open(self):
        if self._h is None or self.env.closed:
            raise RuntimeError("CarDrivers (or its env) is closed")

    def close(self):
        if self._h is not None:
            if not self.env.closed:
                torch.cuda.synchronize(self.device)
            self._L.crl_car_driver_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- styles
    def style_names(self):
        return tuple(sorted(self._slots, key=self._slots.get))

    def slot_of(self, name):
        if name not in self._slots:
            raise ValueError(f"Unknown car driver style {name!r}; known: {self.style_names()}")
        return self._slots[name]

    def _push_style(self, slot, s):
        N.check(self._L.crl_car_driver_set_style(self._h, slot, CAR_DRIVER_KINDS.index(s["kind"]), s["target_speed"], s["lookahead"],
                                                 s["steer_gain"], s["epsilon"]))

    def set_style(self, name, kind="RULE_BASED", **params):
        """Define or redefine style ``name``: ``kind`` RANDOM or RULE_BASED; ``target_speed``, ``lookahead``, ``steer_gain``, ``epsilon``
        (missing ones are the default style's).  Takes effect from the next ``act``; returns the style's slot."""
        self._check_open()
        if not isinstance(name, str) or not name:
            raise ValueError("a style needs a name")
        s = check_car_style(kind, **params)
        if name in CAR_DRIVER_KINDS and s["kind"] != name:
            raise ValueError(f"the built-in style {name} keeps its kind")
        slot = self._slots.get(name, len(self._slots))
        if slot >= N.CRL_CAR_DRIVER_SLOTS:
            raise ValueError(f"all {N.CRL_CAR_DRIVER_SLOTS} style slots are taken")
        self._push_style(slot, s)
        self._slots[name] = slot
        return slot

    def get_style(self, name):
        self._check_open()
        k, la, ts, sg, e = C.c_int32(), C.c_int32(), C.c_float(), C.c_float(), C.c_float()
        N.check(self._L.crl_car_driver_get_style(self._h, self.slot_of(name), C.byref(k), C.byref(ts), C.byref(la), C.byref(sg), C.byref(e)))
        return dict(kind=CAR_DRIVER_KINDS[k.value], target_speed=ts.value, lookahead=la.value, steer_gain=sg.value, epsilon=e.value)

    # ---- assignment
    def assign(self, car, who):
        """Who drives car ``car`` (0 or 1): a style name for every env, an int32 device tensor (N,) of style slots (``slot_of``; -1 =
        nobody) per env, or None: nobody -- ``act`` then leaves that car's actions as the caller wrote them.  No synchronisation."""
        self._check_open()
        if not 0 <= int(car) < self.players:
            raise ValueError(f"car must lie in [0, {self.players})")
        # the mirror takes what the device holds first (a copy on the stream): a CarLeague writes column 1 there on its own
        N.check(self._L.crl_car_driver_get_assignment(self._h, C.c_void_p(self._assign.data_ptr()), self._stream()))
        if isinstance(who, torch.Tensor):
            if who.dtype != torch.int32 or who.device != self.device or tuple(who.shape) != (self.num_envs,):
                raise ValueError(f"a per-env assignment is an int32 tensor of shape ({self.num_envs},) on the env's device")
            self._assign[:, int(car)] = who
        else:
            self._assign[:, int(car)] = -1 if who is None else self.slot_of(who)
        N.check(self._L.crl_car_driver_set_assignment(self._h, C.c_void_p(self._assign.data_ptr()), self._stream()))

    def assignment(self):
        """The assignment as the device holds it: int32 (N, players)."""
        self._check_open()
        out = torch.empty_like(self._assign)
        N.check(self._L.crl_car_driver_get_assignment(self._h, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    # ---- serving
    def act(self, actions):
        """Fill the assigned cars' rows of ``actions`` (float32 (N, players, 2), contiguous, on the env's device) in place from the
        env's current state: enqueued behind the env's last ``reset`` / ``step_device`` on the current stream, no synchronisation."""
        self._check_open()
        if not (isinstance(actions, torch.Tensor) and actions.dtype == torch.float32 and actions.device == self.device
                and actions.is_contiguous() and tuple(actions.shape) == (self.num_envs, self.players, 2)):
            raise AssertionError(f"act needs a contiguous float32 tensor of shape ({self.num_envs}, {self.players}, 2) on the env's device")
        N.check(self._L.crl_car_driver_act(self._h, C.c_void_p(actions.data_ptr()), self._stream()))
        return actions

    # ---- checkpoint / resume
    def _counters(self):
        seed, calls = C.c_uint64(), C.c_int64()
        N.check(self._L.crl_car_driver_get_counters(self._h, C.byref(seed), C.byref(calls)))
        return seed.value, calls.value

    @property
    def calls(self):
        return self._counters()[1]

    def state_dict(self):
        self._check_open()
        seed, calls = self._counters()
        styles = {name: dict(self.get_style(name), slot=slot) for name, slot in self._slots.items()}
        return {"kind": "CarDrivers", "num_envs": self.num_envs, "players": self.players, "seed": seed, "calls": calls, "styles": styles,
                "assignment": self.assignment().cpu().numpy()}

    def load_state_dict(self, sd):
        """Styles, assignment, key and call counter of a ``state_dict()``; everything is looked at before anything is written."""
        self._check_open()
        what = "CarDrivers"
        ck.check_header(sd, "CarDrivers", what, num_envs=self.num_envs, players=self.players)
        seed, calls = ck.check_counter(sd.get("seed"), 64, "seed", what), ck.check_counter(sd.get("calls"), 32, "calls", what)
        assign = ck.check_array(sd, "assignment", (self.num_envs, self.players), 4, what).view(np.int32)
        styles = sd.get("styles")
        if not isinstance(styles, dict) or len(styles) > N.CRL_CAR_DRIVER_SLOTS:
            raise ck.refuse(f"{what}: styles must be a dict of at most {N.CRL_CAR_DRIVER_SLOTS} entries")
        parsed = {}
        for name, s in styles.items():
            try:
                slot = int(s["slot"])
                parsed[name] = (slot, check_car_style(s["kind"], s["target_speed"], int(s["lookahead"]), s["steer_gain"], s["epsilon"]))
            except (KeyError, TypeError, ValueError) as e:
                raise ck.refuse(f"{what}: style {name!r}: {e}") from None
            if not 0 <= slot < N.CRL_CAR_DRIVER_SLOTS:
                raise ck.refuse(f"{what}: style {name!r} sits in slot {slot}")
        slots = sorted(v[0] for v in parsed.values())
        if slots != list(range(len(slots))) or any(parsed.get(k, (None,))[0] != i for i, k in enumerate(CAR_DRIVER_KINDS)):
            raise ck.refuse(f"{what}: the styles must fill slots 0.. without gaps, RANDOM and RULE_BASED in slots 0 and 1")
        for name, (slot, s) in parsed.items():
            self._push_style(slot, s)
        self._slots = {name: slot for name, (slot, _) in parsed.items()}
        self._assign.copy_(torch.as_tensor(np.ascontiguousarray(assign)))
        N.check(self._L.crl_car_driver_set_assignment(self._h, C.c_void_p(self._assign.data_ptr()), self._stream()))
        N.check(self._L.crl_car_driver_set_counters(self._h, seed, calls))
