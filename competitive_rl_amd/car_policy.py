"""Learned CarRacing drivers served on the device (include/crl.h "car policy"): a 21-float state observation per car and the
reference's ``MLP(input_size, output_size)`` (utils/network.py:59-70) on it, assignable per env and per car from a pool of weight sets,
with Gaussian actions, values and log-probabilities -- for CarRacing what ``Policy`` with a critic is for Pong.

The env loop stays on the device, and so does the learner's: ``CarRolloutStorage`` keeps what ``act_rollout`` wrote and ``CarPPO``
updates the weights from it (car_learner.py); a trainer with its own torch network takes (B, 21) minibatches from the storage's
``gather`` / ``minibatches`` instead:

    env = HipCarVecEnv(n)
    policy = CarPolicy(env, seed=0)
    policy.add_network("learner", mlp.state_dict())     # a torch MLP(21, 2), a dict of arrays, or a checkpoint path
    policy.assign(0, "learner")
    storage = CarRolloutStorage(env, steps, cars=(0,))
    actions = torch.zeros((n, 2, 2), device=env.device)
    obs = torch.empty((n, 2, 21), device=env.device)
    env.reset()
    storage.begin()
    values, log_probs = policy.act_rollout(actions, obs_out=obs)
    for t in range(steps):
        storage.record(t, policy, "learner", obs, actions, values, log_probs)   # what the learner's update will see
        _, rewards, done = env.step_device(actions, render=False)
        storage.outcome(t, rewards, done)
        values, log_probs = policy.act_rollout(actions, obs_out=obs)
    storage.finish(values)
    policy.update_network("learner", mlp.state_dict())  # on the stream, no device synchronisation (CarPPO.push: no host blob either)

It composes with ``CarDrivers`` on one action tensor: ``drivers.act(a); policy.act(a)``, each writing only the cars assigned to it.
"""
import ctypes as C

import numpy as np
import torch

from . import _native as N
from . import checkpoint as ck
from .rules import CAR_POLICY_KEYS, car_policy_pack, car_policy_unpack, car_policy_weights

__all__ = ["CarPolicy"]


class CarPolicy:
    def __init__(self, env, seed=0):
        env = getattr(env, "env", env)  # (a HipCompetitiveCarVecEnv wraps its HipCarVecEnv)
        if not hasattr(env, "_h") or not hasattr(env, "P"):
            raise TypeError("CarPolicy needs a HipCarVecEnv")
        env._check_open()
        self.env, self._L = env, env._L
        self.num_envs, self.players, self.device = env.num_envs, env.P, env.device
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._L.crl_car_policy_create(env._h, int(seed) & (2 ** 64 - 1), C.byref(h)))
        self._h = h
        self._slots = {}  # network name -> slot
        self._assign = torch.full((self.num_envs, self.players), -1, dtype=torch.int32, device=self.device)

    # ---- plumbing
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _check_open(self):
        if self._h is None or self.env.closed:
            raise RuntimeError("CarPolicy (or its env) is closed")

    def close(self):
        if self._h is not None:
            if not self.env.closed:
                torch.cuda.synchronize(self.device)
            self._L.crl_car_policy_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- networks
    def network_names(self):
        return tuple(sorted(self._slots, key=self._slots.get))

    def slot_of(self, name):
        if name not in self._slots:
            raise ValueError(f"Unknown car policy network {name!r}; known: {self.network_names()}")
        return self._slots[name]

    def _push(self, slot, blob, deterministic):
        """The blob of a slot, host array -> pinned stage -> device on the current stream: the host waits for neither copy (both
        staging tensors belong to torch's caching allocators, which hand a block out again only behind its last use on the stream)."""
        dev = torch.from_numpy(blob).pin_memory().to(self.device, non_blocking=True)
        N.check(self._L.crl_car_policy_set_weights(self._h, slot, C.c_void_p(dev.data_ptr()), int(bool(deterministic)), self._stream()))

    def add_network(self, name, weights, deterministic=False):
        """A new network ``name``: anything ``rules.car_policy_weights`` takes (a dict of the seven arrays, a torch ``MLP(21, 2)`` state
        dict as it is, or a checkpoint path).  ``deterministic``: act with the mean instead of sampling.  Returns its slot."""
        self._check_open()
        if not isinstance(name, str) or not name:
            raise ValueError("a network needs a name")
        if name in self._slots:
            raise ValueError(f"network {name!r} exists: update_network replaces its weights")
        if len(self._slots) >= N.CRL_CAR_POLICY_SLOTS:
            raise ValueError(f"all {N.CRL_CAR_POLICY_SLOTS} network slots are taken")
        blob = car_policy_pack(weights)
        slot = len(self._slots)
        self._push(slot, blob, deterministic)
        self._slots[name] = slot
        return slot

    def update_network(self, name, weights):
        """New weights for ``name``, copied on the current stream: no device synchronisation; every ``act`` enqueued on that stream
        after this call runs the new weights.  The sampling flag stays."""
        self._check_open()
        slot = self.slot_of(name)
        self._push(slot, car_policy_pack(weights), self.is_deterministic(name))

    def _blob(self, slot):
        out = torch.empty((N.CRL_CAR_POLICY_BLOB_FLOATS,), dtype=torch.float32, device=self.device)
        flag = C.c_int32()
        N.check(self._L.crl_car_policy_get_weights(self._h, slot, C.c_void_p(out.data_ptr()), C.byref(flag), self._stream()))
        return out.cpu().numpy(), bool(flag.value)

    def network_weights(self, name):
        """The seven arrays of ``name`` as the device holds them (a host read: it waits for the current stream)."""
        self._check_open()
        return car_policy_unpack(self._blob(self.slot_of(name))[0])

    def is_deterministic(self, name):
        self._check_open()
        flag = C.c_int32()
        N.check(self._L.crl_car_policy_get_weights(self._h, self.slot_of(name), None, C.byref(flag), None))
        return bool(flag.value)

    def set_sampling(self, name, deterministic):
        """Act with the mean (``deterministic=True``) or sample, from the next ``act`` on."""
        self._check_open()
        N.check(self._L.crl_car_policy_set_sampling(self._h, self.slot_of(name), int(bool(deterministic))))

    # ---- assignment
    def assign(self, car, who):
        """Who drives car ``car`` (0 or 1): a network name for every env, an int32 device tensor (N,) of slots (``slot_of``; -1 =
        nobody) per env, or None: nobody -- ``act`` then leaves that car's actions as the caller wrote them.  No synchronisation."""
        self._check_open()
        if not 0 <= int(car) < self.players:
            raise ValueError(f"car must lie in [0, {self.players})")
        # the mirror takes what the device holds first (a copy on the stream): a CarLeague writes column 1 there on its own
        N.check(self._L.crl_car_policy_get_assignment(self._h, C.c_void_p(self._assign.data_ptr()), self._stream()))
        if isinstance(who, torch.Tensor):
            if who.dtype != torch.int32 or who.device != self.device or tuple(who.shape) != (self.num_envs,):
                raise ValueError(f"a per-env assignment is an int32 tensor of shape ({self.num_envs},) on the env's device")
            self._assign[:, int(car)] = who
        else:
            self._assign[:, int(car)] = -1 if who is None else self.slot_of(who)
        N.check(self._L.crl_car_policy_set_assignment(self._h, C.c_void_p(self._assign.data_ptr()), self._stream()))

    def assignment(self):
        """The assignment as the device holds it: int32 (N, players)."""
        self._check_open()
        out = torch.empty_like(self._assign)
        N.check(self._L.crl_car_policy_get_assignment(self._h, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    # ---- serving
    def _out(self, t, shape, what):
        if t is None:
            return None
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == self.device and t.is_contiguous()
                and tuple(t.shape) == shape):
            raise AssertionError(f"{what} needs a contiguous float32 tensor of shape {shape} on the env's device")
        return t

    def _act(self, actions, values, log_probs, noise, obs):
        n, p = self.num_envs, self.players
        self._out(actions, (n, p, 2), "actions")
        if actions is None:
            raise AssertionError(f"actions needs a contiguous float32 tensor of shape {(n, p, 2)} on the env's device")
        self._out(noise, (n, p, 2), "noise_out"), self._out(obs, (n, p, N.CRL_CAR_OBS_FEATURES), "obs_out")
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
        N.check(self._L.crl_car_policy_act(self._h, ptr(actions), ptr(values), ptr(log_probs), ptr(noise), ptr(obs), self._stream()))

    def act(self, actions):
        """Fill the assigned cars' rows of ``actions`` (float32 (N, players, 2), contiguous, on the env's device) in place from the
        env's current state: one launch on the current stream, no synchronisation.  The actions are not clipped: the env clips."""
        self._check_open()
        self._act(actions, None, None, None, None)
        return actions

    def act_rollout(self, actions, obs_out=None, noise_out=None):
        """``act`` that also returns what a trainer stores: (values, log_probs), float32 (N, players) each, 0 for a car nobody serves
        (and for a done car).  ``obs_out`` (N, players, 21) receives the observation of every car, ``noise_out`` (N, players, 2) the
        standard normal draws z behind the sampled actions (u = mean + std * z)."""
        self._check_open()
        values = torch.empty((self.num_envs, self.players), dtype=torch.float32, device=self.device)
        log_probs = torch.empty_like(values)
        self._act(actions, values, log_probs, noise_out, obs_out)
        return values, log_probs

    def observe(self, out=None):
        """The observation of every car, float32 (N, players, 21) on the device; no network runs and no draw is consumed."""
        self._check_open()
        shape = (self.num_envs, self.players, N.CRL_CAR_OBS_FEATURES)
        out = torch.empty(shape, dtype=torch.float32, device=self.device) if out is None else self._out(out, shape, "out")
        N.check(self._L.crl_car_policy_observe(self._h, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    # ---- checkpoint / resume
    def _counters(self):
        seed, calls = C.c_uint64(), C.c_int64()
        N.check(self._L.crl_car_policy_get_counters(self._h, C.byref(seed), C.byref(calls)))
        return seed.value, calls.value

    @property
    def calls(self):
        return self._counters()[1]

    def state_dict(self):
        self._check_open()
        seed, calls = self._counters()
        networks = {}
        for name, slot in self._slots.items():
            blob, flag = self._blob(slot)
            networks[name] = dict(slot=slot, deterministic=flag, weights=car_policy_unpack(blob))
        return {"kind": "CarPolicy", "num_envs": self.num_envs, "players": self.players, "seed": seed, "calls": calls,
                "networks": networks, "assignment": self.assignment().cpu().numpy()}

    def load_state_dict(self, sd):
        """Networks, flags, assignment, key and call counter of a ``state_dict()``; everything is looked at before anything is
        written: a refused load raises ``ValueError`` and leaves the object as it was."""
        self._check_open()
        what = "CarPolicy"
        ck.check_header(sd, "CarPolicy", what, num_envs=self.num_envs, players=self.players)
        seed, calls = ck.check_counter(sd.get("seed"), 64, "seed", what), ck.check_counter(sd.get("calls"), 32, "calls", what)
        assign = ck.check_array(sd, "assignment", (self.num_envs, self.players), 4, what).view(np.int32)
        networks = sd.get("networks")
        if not isinstance(networks, dict) or len(networks) > N.CRL_CAR_POLICY_SLOTS:
            raise ck.refuse(f"{what}: networks must be a dict of at most {N.CRL_CAR_POLICY_SLOTS} entries")
        parsed = {}
        for name, net in networks.items():
            try:
                slot, flag = int(net["slot"]), net["deterministic"]
                blob = car_policy_pack({k: net["weights"][k] for k in CAR_POLICY_KEYS})
            except (KeyError, TypeError, ValueError) as e:
                raise ck.refuse(f"{what}: network {name!r}: {e}") from None
            if not isinstance(flag, (bool, np.bool_)):
                raise ck.refuse(f"{what}: network {name!r}: deterministic must be a bool, not {flag!r}")
            parsed[name] = (slot, bool(flag), blob)
        if sorted(v[0] for v in parsed.values()) != list(range(len(parsed))):
            raise ck.refuse(f"{what}: the networks must fill slots 0.. without gaps")
        if len(parsed) < len(self._slots):
            raise ck.refuse(f"{what}: the state dict holds {len(parsed)} networks, this object already {len(self._slots)}")
        for name, (slot, flag, blob) in parsed.items():
            self._push(slot, blob, flag)
        self._slots = {name: slot for name, (slot, _, _) in parsed.items()}
        self._assign.copy_(torch.as_tensor(np.ascontiguousarray(assign)))
        N.check(self._L.crl_car_policy_set_assignment(self._h, C.c_void_p(self._assign.data_ptr()), self._stream()))
        N.check(self._L.crl_car_policy_set_counters(self._h, seed, calls))


def is_car_policy_weights(x):
    """Does ``x`` look like MLP weights rather than a driver's name: a dict, or the path of an existing file?"""
    import os

    return isinstance(x, (dict, os.PathLike)) or (isinstance(x, str) and os.path.isfile(x))
