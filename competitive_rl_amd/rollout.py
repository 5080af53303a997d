"""A learner's rollout storage on the device (include/crl.h "rollout storage", csrc/pong_rollout.hip).

Stands in for what a PPO / A2C trainer around the reference keeps between ``trainer.compute_action`` and its update: T steps of stacked
observations as ``FrameStackTensor`` holds them (float32, 28 224 bytes per env and step, utils/utils.py:145-173), actions, log-probs,
values, rewards and dones, then returns and advantages, then shuffled minibatches for the trainer's own torch network.  ``RolloutStorage``
keeps ONE new 42 x 42 uint8 plane per env and step -- the other three planes of a step's stack are the planes of the three steps before
it -- and rebuilds the float32 (or uint8) stack of every sample in the gather kernel:

    storage = RolloutStorage(num_steps, num_envs)
    storage.begin(policy)
    for t in range(num_steps):
        values, actions, logp = policy.act_rollout(obs, reset=done, out=actions2[:, 0])
        storage.record(obs, done, values, actions, logp)
        obs, rew, done = env.step_device(actions2)
        storage.outcome(rew[:, 0], done)
    storage.finish(policy.act_rollout(obs, reset=done)[0])   # (a caller that goes on afterwards feeds this call's frame to the next rollout)
    for batch in storage.minibatches(num_mini_batch):
        batch.obs, batch.actions, batch.old_log_probs, batch.values, batch.returns, batch.advantages

The update itself stays on the device too, for both networks (ppo.py: ``LightPPO``, include/crl.h "ppo update", and ``FullPPO``, "ppo update,
full size"): the gradient is computed from the stored uint8 planes, no float32 stack is gathered, and the new weights reach the served
policy by a device-to-device copy:

    learner = LightPPO(weights_with_critic)                   # FullPPO(...) for Policy(use_light_model=False)
    ...                                                       # the rollout above, storage.finish(...)
    learner.update(storage, num_epochs=4, num_mini_batch=32)  # randperm, grad + step per minibatch, no synchronisation
    learner.push(policy)                                      # and / or learner.push(league, "learner")

Torch allocates, draws the permutation and names the stream; everything else is HIP behind ``crl_rollout_*``.  There is no CPU path.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _native as N
from . import checkpoint as K
from .policy_serving import Policy
from .rules import gae_reference, rollout_stack_reference  # noqa: F401  (re-exported)

RolloutBatch = collections.namedtuple("RolloutBatch", ("obs", "actions", "old_log_probs", "values", "returns", "advantages"))
_OBS_DTYPES = {torch.float32: N.CRL_OBS_F32, torch.uint8: N.CRL_OBS_U8}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class _RolloutBase:
    """What the rollout storages share (``RolloutStorage`` here, ``car_learner.CarRolloutStorage``): the step counters' side of the
    object.  A subclass names its C prefix and what a sample is: ``_total()``, ``gather`` and the arrays of its state dict."""
    _C = "crl_rollout_"  # the C prefix of the storage's calls
    _NSTATS = 2          # the doubles ``stats()`` reads
    _STATES = ("fresh", "active", "finished")

    def _c(self, name):
        return getattr(self._L, self._C + name)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _on_device(self):
        """The storage's calls launch on the device that is current (include/crl.h): every one of them runs inside this."""
        return torch.cuda.device(self.device)

    def _info(self, contents=True):
        """(state, recorded, outcomes, normalised); ``contents``: that of the ``state_dict`` which asks"""
        out = (C.c_int32 * 8)()  # (the car's call appends its sizes)
        N.check(self._c("get_info")(self._h, out))
        if not contents and self._STATES[out[0]] == "active" and out[1]:
            raise ValueError("state_dict(contents=False) in the middle of a rollout would drop the steps recorded so far: pass contents=True")
        return self._STATES[out[0]], out[1], out[2], bool(out[3])

    def _finish(self, last_values):
        with self._on_device():
            N.check(self._c("finish")(self._h, _ptr(last_values), self.gamma, self.gae_lambda, int(self.normalize_advantage), self._stream()))

    def stats(self):
        out = (C.c_double * self._NSTATS)()
        with self._on_device():
            N.check(self._c("stats")(self._h, out))
        return tuple(out)

    def minibatches(self, num_mini_batch, generator=None, **how):
        total = self._total()
        size = total // int(num_mini_batch)
        assert size >= 1, f"{total} samples cannot fill {num_mini_batch} minibatches"
        perm = torch.randperm(total, device=self.device, generator=generator)
        for k in range(int(num_mini_batch)):
            yield self.gather(perm[k * size:(k + 1) * size], **how)

    def _check_state_header(self, sd, **sizes):
        """What ``load_state_dict`` looks at before the arrays: (state, step, outcomes, gamma, gae_lambda, normalize_advantage, contents)"""
        what, T = type(self).__name__, self.num_steps
        K.check_header(sd, what, what, num_steps=T, num_envs=self.num_envs, **sizes)
        state = sd.get("state")
        if state not in self._STATES:
            raise K.refuse(f"{what}: state must be fresh, active or finished, not {state!r}")
        step, outcomes = K.check_counter(sd.get("step"), 31, "step", what), K.check_counter(sd.get("outcomes"), 31, "outcomes", what)
        if step > T or outcomes > step or (state == "finished" and outcomes != T) or (state == "fresh" and step):
            raise K.refuse(f"{what}: step {step} and {outcomes} outcomes do not fit a {state} rollout of {T} steps")
        try:
            gamma, lam, norm = float(sd["gamma"]), float(sd["gae_lambda"]), bool(sd["normalize_advantage"])
        except (KeyError, TypeError, ValueError):
            raise K.refuse(f"{what}: gamma, gae_lambda and normalize_advantage are needed") from None
        c = sd.get("contents")
        if c is None:
            if state == "active" and step:
                raise K.refuse(f"{what}: a state dict without contents cannot continue in the middle of a rollout (step {step})")
        elif not isinstance(c, dict):
            raise K.refuse(f"{what}: contents must be a dict")
        return state, step, outcomes, gamma, lam, norm, c


class RolloutStorage(_RolloutBase):
    def __init__(self, num_steps, num_envs, device=None, gamma=0.99, gae_lambda=0.95, normalize_advantage=True, debug=False):
        """``debug``: assert on the host that every index handed to ``gather`` lies in [0, T * N) -- a device synchronisation per call,
        so not for the hot path, where the validity of the indices is the caller's."""
        if not torch.cuda.is_available():
            raise RuntimeError("competitive_rl_amd.RolloutStorage needs a ROCm GPU; there is no CPU fallback")
        self.num_steps, self.num_envs = int(num_steps), int(num_envs)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.gamma, self.gae_lambda, self.normalize_advantage, self.debug = float(gamma), float(gae_lambda), bool(normalize_advantage), bool(debug)
        self._L = N.load()
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._L.crl_rollout_create(self.device.index or 0, self.num_envs, self.num_steps, C.byref(h)))
        self._h = h
        self.step = 0  # the step the next ``record`` writes

    _total = lambda self: self.num_steps * self.num_envs  # noqa: E731  (the samples a finished storage holds)
    _frames = Policy._frames  # what ``record`` takes as ``obs`` is what ``Policy.act_rollout`` takes (it reads num_envs and device only)

    def close(self):
        if getattr(self, "_h", None):
            self._L.crl_rollout_destroy(self._h)
            self._h = None

    __del__ = close

    def nbytes(self):
        """Device bytes the storage holds: (T + 3) padded planes per env, 27 bytes per env and step, a depth byte per env, the statistics.
        A checkpoint between iterations, ``state_dict(contents=False)``, is 3 * 1764 + 1 = 5 293 host bytes per env whatever T is
        (``state_nbytes``)."""
        t, n = self.num_steps, self.num_envs
        return (t + 3) * n * 1776 + t * n * 27 + n + (2 + 256) * 8

    def _per_env(self, x, dtype, name):
        assert x.device == self.device and x.numel() == self.num_envs and x.shape[0] == self.num_envs and x.dtype in dtype, (
            f"{name}: one {dtype[0]} per env on {self.device}")
        return x

    def _flags(self, x, name):
        x = self._per_env(x, (torch.uint8, torch.bool), name).reshape(-1).contiguous()
        return x.view(torch.uint8) if x.dtype == torch.bool else x

    def begin(self, policy=None):
        """Starts a rollout.  ``policy``: the ``Policy`` whose ``act_rollout`` calls are recorded, BEFORE the call of step 0 -- its
        ``get_stack()`` (or such a uint8 (N, 4, 42, 42) tensor itself) gives the three frames in front of step 0.  None carries the last
        three frames and their masks over from the finished rollout (zeros on a fresh storage)."""
        stack = policy.get_stack() if isinstance(policy, Policy) else policy
        if stack is not None:
            assert stack.device == self.device and stack.dtype == torch.uint8 and tuple(stack.shape) == (self.num_envs, 4, 42, 42), "stack: uint8 (N, 4, 42, 42)"
            stack = stack.contiguous()
        with self._on_device():
            N.check(self._L.crl_rollout_begin(self._h, _ptr(stack), self._stream()))
        self.step = 0

    def record(self, obs, done, values, actions, log_probs):
        """The inputs and outputs of this step's ``policy.act_rollout(obs, reset=done)`` call: ``obs`` and ``done`` (None: no flags) as
        that call took them, ``(values, actions, log_probs)`` as it returned them (``actions``: any int32 view with one element per env,
        e.g. a column of an (N, 2) tensor; values and log-probs float32 (N,); each may be None and is then stored as zeros)."""
        f = self._frames(obs)
        reset = self._flags(done, "done") if done is not None else None
        stride = 1
        if actions is not None:
            self._per_env(actions, (torch.int32,), "actions")
            stride = actions.stride(0) if self.num_envs > 1 else 1
        values = self._per_env(values, (torch.float32,), "values").reshape(-1).contiguous() if values is not None else None
        log_probs = self._per_env(log_probs, (torch.float32,), "log_probs").reshape(-1).contiguous() if log_probs is not None else None
        with self._on_device():
            N.check(self._L.crl_rollout_record(self._h, self.step, _ptr(f), f.stride(0), _ptr(reset), _ptr(actions), stride, _ptr(values),
                                               _ptr(log_probs), self._stream()))
        self.step += 1

    def outcome(self, rewards, done):
        """What the env answered to the step just recorded: ``rewards`` float32, one per env in any strided view (``rew[:, 0]`` of the
        env's (N, 2) reward tensor), ``done`` uint8 / bool (N,)."""
        self._per_env(rewards, (torch.float32,), "rewards")
        stride = rewards.stride(0) if self.num_envs > 1 else 1
        with self._on_device():
            N.check(self._L.crl_rollout_outcome(self._h, self.step - 1, _ptr(rewards), stride, _ptr(self._flags(done, "done")), self._stream()))

    def finish(self, last_values=None):
        """Returns and advantages by GAE (``rules.gae_reference``) and, with ``normalize_advantage``, the advantages' mean and standard
        deviation.  ``last_values``: the critic's values of the observation after the last step, float32 (N,); None: zeros."""
        self._finish(None if last_values is None else self._per_env(last_values, (torch.float32,), "last_values").reshape(-1).contiguous())

    def stats(self):
        """(mean, std) of the advantages as the device computed them, float64.  Synchronises the device: logging and tests."""
        return super().stats()

    # ---- checkpoint / resume (include/crl.h "checkpoint / resume")
    _STEP_FIELDS = (("reset", torch.uint8), ("depth", torch.uint8), ("actions", torch.int32), ("log_probs", torch.float32), ("values", torch.float32))
    _OUTCOME_FIELDS = (("rewards", torch.float32), ("dones", torch.uint8))

    def _copy_state(self, call, info, row0, planes, front_depth, steps, per_step, returns=None, adv=None, stats=None):
        """``crl_rollout_get_state`` / ``_set_state`` over device tensors; ``per_step``: dict name -> tensor or None"""
        f = per_step
        args = [row0, 0 if planes is None else planes.shape[0], _ptr(planes), _ptr(front_depth), steps, _ptr(f.get("reset")), _ptr(f.get("depth")),
                _ptr(f.get("actions")), _ptr(f.get("log_probs")), _ptr(f.get("values")), _ptr(f.get("rewards")), _ptr(f.get("dones")), _ptr(returns), _ptr(adv),
                _ptr(stats), self._stream()]
        with self._on_device():
            N.check(call(self._h, *args) if info is None else call(self._h, info, *args))

    def state_nbytes(self, contents=True):
        """Host bytes of ``state_dict(contents)``'s arrays for a finished rollout: ``contents=False`` is 3 planes and a depth byte per
        env, 3 * 1764 + 1 = 5 293 bytes per env whatever T is; ``contents=True`` adds the T + 3 planes, the front depth and 27 bytes
        per env and step: (T + 6) * 1764 + 2 + 27 T bytes per env."""
        t, n = self.num_steps, self.num_envs
        return n * (3 * 1764 + 1) + (n * ((t + 3) * 1764 + 1 + 27 * t) if contents else 0)

    def state_dict(self, contents=True):
        """Everything a continuation needs, as host arrays (SYNCHRONISES with the current stream).  Always: ``kind``, ``num_steps``,
        ``num_envs``, ``gamma``, ``gae_lambda``, ``normalize_advantage``, ``step``, ``outcomes``, ``state`` (fresh / active / finished),
        ``finished``, and the carry -- what ``begin(None)`` would continue from: ``carry_planes`` uint8 (3, N, 42, 42), oldest first,
        and ``carry_depth`` uint8 (N,), how many of them each env's stack may show; None in the middle of a rollout, where
        ``begin(None)`` is refused.
        ``contents=True`` adds, under ``contents``, everything recorded so far: ``planes`` (step + 3, N, 42, 42) -- the three planes in
        front of step 0, then one per recorded step -- with ``front_depth``, per recorded step ``reset``, ``depth``, ``actions``,
        ``log_probs``, ``values``, per outcome ``rewards`` and ``dones``, and after ``finish`` the ``returns``, the ``advantages``,
        ``adv_mean`` / ``adv_std`` (float64) and whether the finish ``normalized``.  A checkpoint taken in the middle of a rollout, or
        between ``finish`` and ``update``, continues exactly: ``record`` / ``outcome`` of the remaining steps, ``finish``, ``stats()``,
        ``gather``, the learners' ``grad`` and a following ``begin(None)`` give the original's bits.
        ``contents=False`` is the small form for a checkpoint BETWEEN iterations (after the update, before the next ``begin(None)``):
        5 293 bytes per env (``state_nbytes``) instead of ``nbytes()``'s (T + 3) * 1776 + 27 T.  Loaded, the storage stands in front of
        ``begin(None)`` with that carry; what was recorded is gone.  In the middle of a rollout it is refused."""
        state, recorded, outcomes, normalized = self._info(contents)
        T, n, dev = self.num_steps, self.num_envs, self.device
        sd = {"kind": "RolloutStorage", "num_steps": T, "num_envs": n, "gamma": self.gamma, "gae_lambda": self.gae_lambda,
              "normalize_advantage": self.normalize_advantage, "step": self.step, "outcomes": outcomes, "state": state, "finished": state == "finished",
              "carry_planes": None, "carry_depth": None, "contents": None}
        if state != "active" or not recorded:  # the carry of the NEXT rollout: rows T .. T + 2 at min(3, depth[T - 1]) once finished, else the front rows
            planes = torch.empty((3, n, 42, 42), dtype=torch.uint8, device=dev)
            if state == "finished":
                depth = torch.empty((T, n), dtype=torch.uint8, device=dev)
                self._copy_state(self._L.crl_rollout_get_state, None, T, planes, None, T, {"depth": depth})
                depth = depth[T - 1].clamp(max=3)
            else:
                depth = torch.empty((n,), dtype=torch.uint8, device=dev)
                self._copy_state(self._L.crl_rollout_get_state, None, 0, planes, depth, 0, {})
            sd["carry_planes"], sd["carry_depth"] = planes.cpu().numpy(), depth.cpu().numpy()
        if contents:
            planes = torch.empty((recorded + 3, n, 42, 42), dtype=torch.uint8, device=dev)
            front = torch.empty((n,), dtype=torch.uint8, device=dev)
            f = {k: torch.empty((recorded, n), dtype=d, device=dev) for k, d in self._STEP_FIELDS}
            self._copy_state(self._L.crl_rollout_get_state, None, 0, planes, front, recorded, f)
            g = {k: torch.empty((outcomes, n), dtype=d, device=dev) for k, d in self._OUTCOME_FIELDS}
            self._copy_state(self._L.crl_rollout_get_state, None, 0, None, None, outcomes, g)
            c = {"planes": planes.cpu().numpy(), "front_depth": front.cpu().numpy(), **{k: v.cpu().numpy() for k, v in {**f, **g}.items()}}
            if state == "finished":
                ret, adv = (torch.empty((T, n), dtype=torch.float32, device=dev) for _ in range(2))
                stats = torch.zeros((2,), dtype=torch.float64, device=dev)
                self._copy_state(self._L.crl_rollout_get_state, None, 0, None, None, 0, {}, ret, adv, stats if normalized else None)
                stats = stats.cpu().numpy()
                c.update(returns=ret.cpu().numpy(), advantages=adv.cpu().numpy(), adv_mean=float(stats[0]), adv_std=float(stats[1]), normalized=normalized)
            sd["contents"] = c
        return sd

    def load_state_dict(self, sd):
        """Puts a ``state_dict()`` of either form back.  Everything is looked at before anything is written: other T or N, a ``step``
        outside [0, T], arrays of the wrong shape or a carry that is missing raise a ``ValueError`` and leave the storage as it was.
        ``gamma``, ``gae_lambda`` and ``normalize_advantage`` become the dict's.  Ordered on the current stream and SYNCHRONISES with it
        (the staging tensors are the call's own)."""
        T, n, dev, what = self.num_steps, self.num_envs, self.device, "RolloutStorage"
        state, step, outcomes, gamma, lam, norm, c = self._check_state_header(sd)
        np_of = {torch.uint8: 1, torch.int32: 4, torch.float32: 4}
        if c is None:
            planes = K.check_array(sd, "carry_planes", (3, n, 42, 42), 1, what).view(np.uint8)
            front = K.check_array(sd, "carry_depth", (n,), 1, what).view(np.uint8)
            info, recorded, f, g, fin = (C.c_int32 * 4)(0, 0, 0, 0), 0, {}, {}, None
        else:
            recorded = T if state == "finished" else step
            planes = K.check_array(c, "planes", (recorded + 3, n, 42, 42), 1, what).view(np.uint8)
            front = K.check_array(c, "front_depth", (n,), 1, what).view(np.uint8)
            f = {k: K.check_array(c, k, (recorded, n), np_of[d], what) for k, d in self._STEP_FIELDS}
            g = {k: K.check_array(c, k, (outcomes, n), np_of[d], what) for k, d in self._OUTCOME_FIELDS}
            fin, normalized = None, False
            if state == "finished":
                fin = [K.check_array(c, k, (T, n), 4, what).view(np.float32) for k in ("returns", "advantages")]
                normalized = bool(c.get("normalized"))
                try:
                    fin.append(np.array([float(c["adv_mean"]), float(c["adv_std"])], np.float64))
                except (KeyError, TypeError, ValueError):
                    raise K.refuse(f"{what}: adv_mean and adv_std are needed after a finish") from None
            info = (C.c_int32 * 4)(self._STATES.index(state), recorded, outcomes, int(normalized))

        def up(a, dtype):  # (the bits as they are, under the storage's dtype)
            as_np = {torch.uint8: np.uint8, torch.int32: np.int32, torch.float32: np.float32, torch.float64: np.float64}[dtype]
            return torch.from_numpy(np.ascontiguousarray(a).view(as_np).copy()).to(dev)

        fd = {k: up(f[k], d) for k, d in self._STEP_FIELDS if k in f}
        self._copy_state(self._L.crl_rollout_set_state, info, 0, up(planes, torch.uint8), up(front, torch.uint8), recorded, fd)
        if g and outcomes:
            self._copy_state(self._L.crl_rollout_set_state, info, 0, None, None, outcomes, {k: up(g[k], d) for k, d in self._OUTCOME_FIELDS})
        if fin is not None:
            self._copy_state(self._L.crl_rollout_set_state, info, 0, None, None, 0, {}, up(fin[0], torch.float32), up(fin[1], torch.float32),
                             up(fin[2], torch.float64))
        self.step = 0 if c is None else step
        self.gamma, self.gae_lambda, self.normalize_advantage = gamma, lam, norm
        torch.cuda.current_stream(dev).synchronize()  # the staging tensors above are this call's own

    def empty_batch(self, batch_size, obs_dtype=torch.float32, fields=None):
        """Buffers for ``gather(idx, out=...)`` of ``batch_size`` samples; a field not named in ``fields`` is None and is not gathered."""
        want = set(RolloutBatch._fields if fields is None else fields)
        assert want <= set(RolloutBatch._fields) and obs_dtype in _OBS_DTYPES, (fields, obs_dtype)
        b, dev = int(batch_size), self.device
        shapes = {"obs": ((b, 4, 42, 42), obs_dtype), "actions": ((b,), torch.int32), "old_log_probs": ((b,), torch.float32), "values": ((b,), torch.float32),
                  "returns": ((b,), torch.float32), "advantages": ((b,), torch.float32)}
        return RolloutBatch(**{k: torch.empty(s, dtype=d, device=dev) if k in want else None for k, (s, d) in shapes.items()})

    def gather(self, idx, out=None, obs_dtype=torch.float32, fields=None):
        """The samples ``idx`` (int64 on the device, flat ``t * num_envs + e``, any order, duplicates allowed) as a ``RolloutBatch``:
        ``obs`` (B, 4, 42, 42) float32 holding 0..255 (or uint8) -- the stack ``policy.get_stack()`` showed right after the act call of
        step t --, ``actions`` int32, ``old_log_probs``, ``values``, ``returns``, ``advantages`` float32 (B,).  ``out``: a ``RolloutBatch``
        to write into (``empty_batch``), fields that are None are skipped; else new tensors for ``fields`` (default: all)."""
        assert idx.device == self.device and idx.dtype == torch.int64 and idx.dim() == 1, "idx: int64 (B,) on the storage's device"
        idx = idx.contiguous()
        if self.debug:
            assert idx.numel() == 0 or (0 <= int(idx.min()) and int(idx.max()) < self.num_steps * self.num_envs), "idx outside [0, T * N)"
        if out is None:
            out = self.empty_batch(idx.numel(), obs_dtype, fields)
        dtype = obs_dtype
        if out.obs is not None:
            dtype = out.obs.dtype
            assert (dtype in _OBS_DTYPES and out.obs.device == self.device and out.obs.is_contiguous() and
                    tuple(out.obs.shape) == (idx.numel(), 4, 42, 42)), "out.obs: (B, 4, 42, 42) float32 / uint8 on the storage's device"
        for name, t in zip(RolloutBatch._fields[1:], out[1:]):
            assert t is None or (t.is_contiguous() and t.numel() == idx.numel() and t.device == self.device and
                                 t.dtype == (torch.int32 if name == "actions" else torch.float32)), name
        with self._on_device():
            N.check(self._L.crl_rollout_gather(self._h, _ptr(idx), idx.numel(), _ptr(out.obs), _OBS_DTYPES[dtype], _ptr(out.actions),
                                               _ptr(out.old_log_probs), _ptr(out.values), _ptr(out.returns), _ptr(out.advantages), self._stream()))
        return out

    def minibatches(self, num_mini_batch, generator=None, obs_dtype=torch.float32):
        """``num_mini_batch`` batches of T * N // num_mini_batch samples each, drawn without replacement by ``torch.randperm`` on the
        device (``generator``: a device generator, for a reproducible order)."""
        return super().minibatches(num_mini_batch, generator, obs_dtype=obs_dtype)
