"""A CarRacing learner's loop on the device: ``CarRolloutStorage`` (include/crl.h "car rollout storage", csrc/car_rollout.hip) and
``CarPPO`` ("car ppo update", csrc/car_ppo.hip) -- for ``CarPolicy`` what ``RolloutStorage`` and ``LightPPO`` are for ``Policy``.

The observation of a car is 84 bytes, so the whole loop lives on the device; no pixels are drawn and no call synchronises:

    env = HipCarVecEnv(n)
    policy = CarPolicy(env, seed=0)
    learner = CarPPO(mlp.state_dict())                       # a torch MLP(21, 2), a dict of arrays, or a checkpoint path
    policy.add_network("learner", learner.weights())
    policy.assign(0, "learner"), policy.assign(1, "learner")
    storage = CarRolloutStorage(env, num_steps, cars=(0, 1))
    actions = torch.zeros((n, 2, 2), device=env.device)
    obs = torch.empty((n, 2, 21), device=env.device)
    env.reset()
    values, log_probs = policy.act_rollout(actions, obs_out=obs)
    for iteration in range(iterations):
        storage.begin()
        for t in range(num_steps):
            storage.record(t, policy, "learner", obs, actions, values, log_probs)
            _, rewards, done = env.step_device(actions, render=False)
            storage.outcome(t, rewards, done)
            values, log_probs = policy.act_rollout(actions, obs_out=obs)   # opens the next step, or the next rollout
        storage.finish(values)
        learner.update(storage, num_epochs=4, num_mini_batch=8)
        learner.push(policy, "learner")

Torch allocates, draws the permutation and names the stream; everything else is HIP.  There is no CPU path.  The loss, its summation
shape and the optimiser step are the header's written rule; ``rules.car_ppo_loss_reference`` (autograd, float64) and
``rules.adam_reference`` restate them.

Teacher targets (include/crl.h "car ppo update, teacher targets") add ``coef * term`` towards a per-sample target action or mean.
Cloning RULE_BASED by DAgger -- the learner drives, a second ``CarDrivers`` answers every visited state into a scratch tensor:

    rule = CarDrivers(env)
    rule.assign(0, "RULE_BASED"), rule.assign(1, "RULE_BASED")
    target = torch.zeros((num_steps, n, 2, 2), device=env.device)
    for t in range(num_steps):
        rule.act(target[t])                                            # before the step that consumes the learner's action
        storage.record(t, policy, "learner", obs, actions, values, log_probs)
        ...
    learner.update(storage, 4, 8, teacher=CarTeacher(target, loss="mse", policy_term=False))
    print(learner.teacher_stats())                                     # term, kl, abs_err, taught (synchronises)

``CarTeacher(mean_of_a_snapshot, log_std=snapshot_weights, coef=0.1)`` with the policy term left on is PPO held near that snapshot (a
deterministic ``CarPolicy`` slot writes its mean the same way); ``rules.car_ppo_teacher_loss_reference`` restates the loss.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _native as N
from . import checkpoint as K
from .car_policy import CarPolicy
from .ppo import _PPOLearner
from .rollout import _ptr, _RolloutBase
from .rules import (CAR_POLICY_KEYS, CAR_POLICY_SHAPES, CAR_PPO_DEFAULTS, adam_reference, car_policy_pack, car_policy_unpack,  # noqa: F401  (re-exported)
                    car_ppo_loss_reference, car_ppo_teacher_loss_reference, check_car_teacher, gae_reference)

__all__ = ["CarRolloutStorage", "CarRolloutBatch", "CarPPO", "CarPPOStats", "CarTeacher", "CarTeacherStats", "car_blob_views"]

CarRolloutBatch = collections.namedtuple("CarRolloutBatch", ("obs", "actions", "old_log_probs", "values", "returns", "advantages", "live"))
CarPPOStats = collections.namedtuple("CarPPOStats", ("policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "grad_norm", "steps", "live"))
CarTeacherStats = collections.namedtuple("CarTeacherStats", ("term", "kl", "abs_err", "taught"))
LINE_WORDS = 32  # one sample = one aligned 128-byte line
_CARS = {(0,): 1, (1,): 2, (0, 1): 3}


def car_blob_views(blob):
    """The seven tensors of a flat car policy blob (a torch tensor or a numpy array of 2508 floats) as VIEWS in torch layout, by key:
    ``fc1_w`` is the transposed view of the blob's [21][100] block."""
    H, K = N.CRL_CAR_POLICY_HIDDEN, N.CRL_CAR_OBS_FEATURES
    t = K * H + 4 * H
    fc1 = blob[:K * H].reshape(K, H)
    return dict(fc1_w=fc1.t() if isinstance(fc1, torch.Tensor) else fc1.T, fc1_b=blob[K * H:K * H + H], policy_w=blob[K * H + H:K * H + 3 * H].reshape(2, H),
                policy_b=blob[t:t + 2], value_w=blob[K * H + 3 * H:t].reshape(1, H), value_b=blob[t + 2:t + 3], log_std=blob[t + 3:t + 5])


class CarRolloutStorage(_RolloutBase):
    _C, _NSTATS = "crl_car_rollout_", 3
    _total = lambda self: self.num_steps * self.rows  # noqa: E731  (the samples a finished storage holds)

    def __init__(self, env, num_steps, cars=(0,), gamma=0.99, gae_lambda=0.95, normalize_advantage=True):
        """``cars``: which cars' samples are kept, one of (0,), (1,), (0, 1).  Rows R = N * len(cars), row = e * len(cars) + j; the
        flat index of a sample is t * R + row."""
        env = getattr(env, "env", env)  # (a HipCompetitiveCarVecEnv wraps its HipCarVecEnv)
        if not hasattr(env, "_h") or not hasattr(env, "P"):
            raise TypeError("CarRolloutStorage needs a HipCarVecEnv")
        env._check_open()
        cars = tuple(int(c) for c in cars)
        if cars not in _CARS:
            raise ValueError(f"cars must be one of {sorted(_CARS)}, not {cars}")
        self.env, self._L = env, env._L
        self.num_envs, self.players, self.device = env.num_envs, env.P, env.device
        self.num_steps, self.cars = int(num_steps), cars
        self.rows = self.num_envs * len(cars)
        self.gamma, self.gae_lambda, self.normalize_advantage = float(gamma), float(gae_lambda), bool(normalize_advantage)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._L.crl_car_rollout_create(env._h, self.num_steps, _CARS[cars], C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            if not self.env.closed:
                torch.cuda.synchronize(self.device)
            self._L.crl_car_rollout_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def nbytes(self):
        """Device bytes the storage holds: a 128-byte line per sample, the policy's assignment, the statistics."""
        return self.num_steps * self.rows * LINE_WORDS * 4 + self.num_envs * self.players * 4 + (3 + 2 * 256) * 8

    def _full(self, t, tail, what, dtype=torch.float32):
        shape = (self.num_envs, self.players) + tail
        if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.device == self.device and t.is_contiguous() and tuple(t.shape) == shape):
            raise AssertionError(f"{what} needs a contiguous {dtype} tensor of shape {shape} on the env's device")
        return t

    def begin(self):
        """Starts a rollout: there is no frame history to carry, the call only rewinds the step counter."""
        N.check(self._L.crl_car_rollout_begin(self._h))

    def record(self, t, policy, name, obs, actions, values, log_probs):
        """Step ``t``: the full tensors that ``policy.act_rollout(actions, obs_out=obs)`` just wrote -- (N, P, 21), (N, P, 2), (N, P),
        (N, P) -- for network ``name`` of ``policy``.  The storage keeps its cars' columns and ``live``: the car is assigned to
        ``name``, is not done and its env has a track -- the conditions under which ``act_rollout`` served a real sample.  A
        deterministic network is refused: its log-probs are 0."""
        if not isinstance(policy, CarPolicy) or policy.env is not self.env:
            raise ValueError("record needs the CarPolicy of this storage's env")
        self._full(obs, (N.CRL_CAR_OBS_FEATURES,), "obs"), self._full(actions, (2,), "actions")
        self._full(values, (), "values"), self._full(log_probs, (), "log_probs")
        with self._on_device():
            N.check(self._L.crl_car_rollout_record(self._h, int(t), policy._h, policy.slot_of(name), _ptr(obs), _ptr(actions), _ptr(values),
                                                   _ptr(log_probs), self._stream()))

    def outcome(self, t, rewards, done):
        """What the env answered to step ``t``: the (N, P) float32 reward buffer and the (N,) uint8 done buffer as ``step_device``
        returns them.  A row's done is ``done[e] != 0 or done_car[e][c] != 0`` (the env's own per-car flags)."""
        self._full(rewards, (), "rewards")
        if not (isinstance(done, torch.Tensor) and done.dtype in (torch.uint8, torch.bool) and done.device == self.device and
                done.is_contiguous() and tuple(done.shape) == (self.num_envs,)):
            raise AssertionError(f"done needs a contiguous uint8 tensor of shape ({self.num_envs},) on the env's device")
        with self._on_device():
            N.check(self._L.crl_car_rollout_outcome(self._h, int(t), _ptr(rewards), _ptr(done), self._stream()))

    def finish(self, last_values=None):
        """Returns and advantages by GAE (``rules.gae_reference`` with the rows' dones) and, with ``normalize_advantage``, the mean and
        the unbiased deviation of the LIVE samples' advantages.  ``last_values``: (N, P), the values of the ``act_rollout`` call that
        opens the next rollout; None: zeros."""
        self._finish(None if last_values is None else self._full(last_values, (), "last_values"))

    def stats(self):
        """(mean, std, live count) of the advantages as the device computed them.  Synchronises the device: logging and tests."""
        mean, std, live = super().stats()
        return mean, std, int(live)

    # ---- minibatches
    def empty_batch(self, batch_size, fields=None):
        """Buffers for ``gather(idx, out=...)``; a field not named in ``fields`` is None and is not gathered."""
        want = set(CarRolloutBatch._fields if fields is None else fields)
        assert want <= set(CarRolloutBatch._fields), fields
        b, dev, f = int(batch_size), self.device, torch.float32
        shapes = {"obs": ((b, N.CRL_CAR_OBS_FEATURES), f), "actions": ((b, 2), f), "old_log_probs": ((b,), f), "values": ((b,), f), "returns": ((b,), f),
                  "advantages": ((b,), f), "live": ((b,), torch.uint8)}
        return CarRolloutBatch(**{k: torch.empty(s, dtype=d, device=dev) if k in want else None for k, (s, d) in shapes.items()})

    def gather(self, idx, out=None, fields=None):
        """The samples ``idx`` (int64 on the device, flat ``t * rows + row``, any order, duplicates allowed) as a ``CarRolloutBatch``:
        obs (B, 21), actions (B, 2), old log-probs, values, returns, advantages float32 (B,), live uint8 (B,)."""
        assert idx.device == self.device and idx.dtype == torch.int64 and idx.dim() == 1, "idx: int64 (B,) on the storage's device"
        idx = idx.contiguous()
        if out is None:
            out = self.empty_batch(idx.numel(), fields)
        for name, t in zip(CarRolloutBatch._fields, out):
            assert t is None or (t.is_contiguous() and t.shape[0] == idx.numel() and t.device == self.device and
                                 t.dtype == (torch.uint8 if name == "live" else torch.float32)), name
        with self._on_device():
            N.check(self._L.crl_car_rollout_gather(self._h, _ptr(idx), idx.numel(), *[_ptr(t) for t in out], self._stream()))
        return out

    def minibatches(self, num_mini_batch, generator=None):
        """``num_mini_batch`` batches of T * R // num_mini_batch samples each, drawn without replacement by ``torch.randperm``."""
        return super().minibatches(num_mini_batch, generator)

    # ---- checkpoint / resume
    def state_dict(self, contents=True):
        """Everything a continuation needs, as host arrays (SYNCHRONISES with the current stream): the sizes, ``gamma``, ``gae_lambda``,
        ``normalize_advantage``, ``state`` (fresh / active / finished), ``step`` and ``outcomes``.  ``contents=True`` adds, under
        ``contents``, the recorded steps' sample lines as they are (``lines`` uint32 (step * rows, 32)) and after a normalising finish
        the three statistics: a checkpoint taken in the middle of a rollout, or between ``finish`` and ``update``, continues exactly.
        ``contents=False`` is the small form for a checkpoint BETWEEN iterations -- nothing carries over from one rollout to the next,
        so it holds no array; loaded, the storage stands in front of ``begin()``.  In the middle of a rollout it is refused."""
        state, recorded, outcomes, normalized = self._info(contents)
        sd = {"kind": "CarRolloutStorage", "num_steps": self.num_steps, "num_envs": self.num_envs, "players": self.players, "cars": self.cars,
              "gamma": self.gamma, "gae_lambda": self.gae_lambda, "normalize_advantage": self.normalize_advantage, "state": state, "step": recorded,
              "outcomes": outcomes, "contents": None}
        if contents:
            lines = torch.empty((recorded * self.rows, LINE_WORDS), dtype=torch.float32, device=self.device)
            stats = torch.zeros((3,), dtype=torch.float64, device=self.device)
            with self._on_device():
                N.check(self._L.crl_car_rollout_get_state(self._h, recorded, _ptr(lines), _ptr(stats), self._stream()))
            sd["contents"] = {"lines": lines.cpu().numpy().view(np.uint32), "stats": stats.cpu().numpy(), "normalized": normalized}
        return sd

    def load_state_dict(self, sd):
        """Puts a ``state_dict()`` of either form back.  Everything is looked at before anything is written: other sizes or cars, a
        ``step`` outside [0, T] or arrays of the wrong shape raise a ``ValueError`` and leave the storage as it was.  Ordered on the
        current stream and SYNCHRONISES with it."""
        what, T = "CarRolloutStorage", self.num_steps
        state, step, outcomes, gamma, lam, norm, c = self._check_state_header(sd, players=self.players)
        if tuple(sd.get("cars", ())) != self.cars:
            raise K.refuse(f"{what}: cars is {sd.get('cars')!r} in the state dict and {self.cars!r} here")
        if state == "finished" and step != T:
            raise K.refuse(f"{what}: step {step} and {outcomes} outcomes do not fit a finished rollout of {T} steps")
        if c is None:
            info, lines, stats, step = (C.c_int32 * 4)(0, 0, 0, 0), None, None, 0
        else:
            lines = K.check_array(c, "lines", (step * self.rows, LINE_WORDS), 4, what)
            stats = K.check_array(c, "stats", (3,), 8, what)
            info = (C.c_int32 * 4)(self._STATES.index(state), step, outcomes, int(bool(c.get("normalized"))))
            lines = torch.from_numpy(np.ascontiguousarray(lines).view(np.float32).copy()).to(self.device)
            stats = torch.from_numpy(np.ascontiguousarray(stats).view(np.float64).copy()).to(self.device)
        with self._on_device():
            N.check(self._L.crl_car_rollout_set_state(self._h, info, step, _ptr(lines), _ptr(stats), self._stream()))
        self.gamma, self.gae_lambda, self.normalize_advantage = gamma, lam, norm
        torch.cuda.current_stream(self.device).synchronize()  # the staging tensors above are this call's own


class CarTeacher:
    """Teacher targets for ``CarPPO.grad`` / ``update`` (include/crl.h "car ppo update, teacher targets"): a small value object over the
    CALLER's tensors, like ``ppo.Teacher`` -- they are not learner state, and the learner keeps no reference beyond the call.
      target         float32 (T*R, 2), (T, R, 2) or (T, N, C, 2): the teacher's action or mean for every stored sample; a row with a
                     NaN or an infinity has no teacher term
      log_std        None: a point teacher (RULE_BASED, a network's mean taken as it is); a pair of floats, or a car policy weight
                     dict or blob whose ``log_std`` is taken: the Gaussian teacher N(target, exp(log_std)^2)
      loss           "ce": E_q[-log p], for a point teacher the Gaussian negative log-likelihood of the target; "mse":
                     0.5 |mean - target|^2, which leaves log_std to the other terms
      value_targets  optionally float32 (T*R,), (T, R) or (T, N, C) in place of the stored returns (a teacher's critic)
    All contiguous, on the learner's device, row ``t * R + row`` the sample ``storage.gather`` calls so.  The loss per live sample
    becomes ``policy_term * policy + vf * value - ent * entropy + coef * term``: ``policy_term=False`` is pure imitation, ``coef=0``
    with ``policy_term=True`` the plain PPO loss.  A wrong type, dtype or shape raises a ``ValueError`` here; the device and the row
    count are checked against the learner and the storage by ``grad``, before any native call."""

    def __init__(self, target, log_std=None, loss="ce", value_targets=None, coef=1.0, policy_term=True):
        self.point, self.log_std, self.kind, self.coef, self.policy_term = check_car_teacher(log_std, loss, coef, policy_term)
        self.loss, self.target, self.value_targets = loss, target, value_targets
        rows = set()
        for name, t, tail in (("target", target, (2,)), ("value_targets", value_targets, ())):
            if t is None and name != "target":
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise ValueError(f"CarTeacher: {name} must be a torch.float32 tensor")
            lead = t.shape[:t.dim() - len(tail)]
            if tuple(t.shape[t.dim() - len(tail):]) != tail or len(lead) not in (1, 2, 3) or not t.is_contiguous():
                raise ValueError(f"CarTeacher: {name} must be contiguous (T*R, ...), (T, R, ...) or (T, N, C, ...) with trailing shape {tail}, "
                                 f"not {tuple(t.shape)}")
            if t.data_ptr() % (8 if tail else 4):
                raise ValueError(f"CarTeacher: {name} must start on a multiple of {8 if tail else 4} bytes")
            rows.add(int(np.prod(lead)))
        if len(rows) != 1:
            raise ValueError(f"CarTeacher: the tensors hold different numbers of samples ({sorted(rows)})")
        self.rows = rows.pop()

    def _tensors(self):
        return [t for t in (self.target, self.value_targets) if t is not None]

    def _native(self, device, total):
        """the crl_car_ppo_teacher of this teacher for a learner on ``device`` and a storage of ``total`` samples"""
        for t in self._tensors():
            if t.device != device:
                raise ValueError(f"CarTeacher: a tensor lives on {t.device}, the learner on {device}")
        if self.rows != total:
            raise ValueError(f"CarTeacher: {self.rows} rows, but the storage holds T * R = {total} samples")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        return N.CrlCarPpoTeacher(ptr(self.target), ptr(self.value_targets), self.rows, (C.c_float * 2)(*self.log_std), self.point, self.kind,
                                  self.coef, self.policy_term)


class CarPPO(_PPOLearner):
    """``ppo._PPOLearner`` over ``crl_car_ppo_*``: hyper-parameters, ``step``, ``close`` and the optimiser half of the state dict are
    the base's; here is what the MLP(21, 2) and its line storage make different."""
    _C, _DEFAULTS, _FLOATS, _SIZED = "crl_car_ppo_", CAR_PPO_DEFAULTS, N.CRL_CAR_POLICY_BLOB_FLOATS, False
    _TEACHER = CarTeacher
    _views = staticmethod(car_blob_views)
    _split = staticmethod(car_policy_unpack)

    def __init__(self, weights, device=None, **hyper):
        """``weights``: anything ``rules.car_policy_weights`` takes (a dict of the seven arrays, a torch ``MLP(21, 2)`` state dict, a
        checkpoint path).  ``hyper``: ``clip``, ``vf_coef``, ``ent_coef``, ``lr``, ``betas``, ``eps``, ``max_grad_norm``
        (``rules.CAR_PPO_DEFAULTS``, common continuous-control practice); the dict ``hyper`` may be changed between calls."""
        self._open(device, hyper)
        blob = car_policy_pack(weights)
        self._L = N.load()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._L.crl_car_ppo_create(self.device.index or 0, blob.ctypes.data_as(C.c_void_p), C.byref(h)))
        self._h = h

    def grad(self, storage, idx, teacher=None):
        """The gradient of the loss over the samples ``idx`` (int64 on the device, as ``storage.gather`` takes them) of a finished
        ``CarRolloutStorage``, at the learner's weights: a dict of device VIEWS of the seven gradient tensors in torch layout, for
        callers with their own optimiser (``grad_blob()``: the same memory as one flat blob); the next ``grad`` overwrites them.
        ``teacher``: a ``CarTeacher`` adds its term to the loss (``teacher_stats()`` then has its statistics); None is the plain PPO
        loss.  A teacher of the wrong type, device or row count raises a ``ValueError`` and changes nothing.  No synchronisation."""
        return super().grad(storage, idx, teacher)

    def grad_blob(self):
        """The last gradient as a device VIEW of the learner's own memory: float32 (2508,) in the weights' layout (include/crl.h "car
        policy"; the std floats and the pad are 0).  No synchronisation."""
        p = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._L.crl_car_ppo_get_grad(self._h, C.byref(p), None))
        return self._dev_blob(p.value)

    def step(self):
        """Clips the last gradient to ``max_grad_norm`` and takes one Adam step on the master weights, in place; the two std floats of
        the blob follow the new log_std.  No synchronisation."""
        super().step()

    def update(self, storage, num_epochs, num_mini_batch, generator=None, teacher=None):
        """``num_epochs`` passes over the finished ``storage``: per pass one ``torch.randperm`` on the device cut into
        ``num_mini_batch`` batches of T * R // num_mini_batch samples, ``grad`` and ``step`` per batch; ``teacher`` goes to every
        ``grad``.  Nothing synchronises."""
        super().update(storage, num_epochs, num_mini_batch, generator, teacher)

    def teacher_stats(self):
        """``CarTeacherStats`` of the last ``grad`` with a teacher: the means over the taught samples of the teacher term, of
        KL(teacher || learner) (a Gaussian teacher under "ce"; otherwise 0) and of the mean's absolute error per component, and the
        taught share of the live samples.  Refuses after a plain ``grad``.  Synchronises the device: logging and tests."""
        return CarTeacherStats(*super().teacher_stats())

    def push(self, policy, name):
        """The master weights into network ``name`` of a ``CarPolicy``: one device-to-device copy ordered on the current stream, the
        host is not touched; the network's sampling flag stays."""
        assert policy.device == self.device, "the policy lives on another device"
        p = self._blob_dev(policy)
        with torch.cuda.device(self.device):
            N.check(self._L.crl_car_policy_set_weights(policy._h, policy.slot_of(name), p, int(policy.is_deterministic(name)), self._stream()))

    def _blob(self):
        blob = np.empty(self._FLOATS, np.float32)
        with torch.cuda.device(self.device):
            N.check(self._L.crl_car_ppo_get_weights(self._h, blob.ctypes.data_as(C.c_void_p)))
        return blob

    def weights(self):
        """The master weights as the seven float32 arrays of ``rules.CAR_POLICY_KEYS`` in torch layout (synchronises)."""
        return car_policy_unpack(self._blob())

    def set_weights(self, weights):
        """Replaces the master weights and zeroes Adam's moments and step count (synchronises)."""
        blob = car_policy_pack(weights)
        with torch.cuda.device(self.device):
            N.check(self._L.crl_car_ppo_set_weights(self._h, blob.ctypes.data_as(C.c_void_p)))

    def stats(self):
        """``CarPPOStats`` of the last ``grad``: the means over the live samples of policy loss, value loss, entropy,
        ``old_logp - logp`` and the clipped share, the gradient's norm before clipping, the optimiser steps taken and the live count.
        Synchronises the device: logging and tests."""
        out = (C.c_double * 8)()
        with torch.cuda.device(self.device):
            N.check(self._L.crl_car_ppo_stats(self._h, out))
        return CarPPOStats(*out[:6], int(out[6]), int(out[7]))

    # ---- checkpoint / resume: ``state_dict()`` -- the master ``weights`` by key, Adam's moments ``m`` and ``v`` by key (the blob's std
    # floats, which are derived, are not state), ``steps`` and ``hyper`` -- and ``load_state_dict`` are the base's over these tensors
    def _get_state(self):
        w, m, v, steps, _ = self._state()
        return [w, m, v], steps

    def _state_blobs(self, sd):
        blobs = []
        for part in ("weights", "m", "v"):
            try:
                arrays = {k: np.asarray(sd[part][k], np.float32) for k in CAR_POLICY_KEYS}
                if part == "weights":
                    blobs.append(car_policy_pack(arrays))
                else:  # (moments may be any finite or non-finite floats; their std entries and the pad are 0)
                    for k, s in CAR_POLICY_SHAPES.items():
                        if arrays[k].shape != s:
                            raise ValueError(f"{k} has shape {arrays[k].shape}, the MLP's is {s}")
                    b = np.concatenate([arrays["fc1_w"].T.reshape(-1), arrays["fc1_b"], arrays["policy_w"].reshape(-1), arrays["value_w"].reshape(-1),
                                        arrays["policy_b"], arrays["value_b"], arrays["log_std"], np.zeros(3, np.float32)]).astype(np.float32)
                    blobs.append(np.ascontiguousarray(b))
            except (KeyError, TypeError, ValueError) as e:
                raise K.refuse(f"CarPPO {part}: {e}") from None
        return blobs
