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

import torch

from . import _native as N
from .policy_serving import Policy
from .rules import gae_reference, rollout_stack_reference  # noqa: F401  (re-exported)

RolloutBatch = collections.namedtuple("RolloutBatch", ("obs", "actions", "old_log_probs", "values", "returns", "advantages"))
_OBS_DTYPES = {torch.float32: N.CRL_OBS_F32, torch.uint8: N.CRL_OBS_U8}


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class RolloutStorage:
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

    _frames = Policy._frames  # what ``record`` takes as ``obs`` is what ``Policy.act_rollout`` takes (it reads num_envs and device only)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _on_device(self):
        """The ``crl_rollout_*`` calls launch on the device that is current (include/crl.h): every one of them runs inside this."""
        return torch.cuda.device(self.device)

    def close(self):
        if getattr(self, "_h", None):
            self._L.crl_rollout_destroy(self._h)
            self._h = None

    __del__ = close

    def nbytes(self):
        """Device bytes the storage holds: (T + 3) padded planes per env, 27 bytes per env and step, a depth byte per env, the statistics."""
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
        if last_values is not None:
            last_values = self._per_env(last_values, (torch.float32,), "last_values").reshape(-1).contiguous()
        with self._on_device():
            N.check(self._L.crl_rollout_finish(self._h, _ptr(last_values), self.gamma, self.gae_lambda, int(self.normalize_advantage), self._stream()))

    def stats(self):
        """(mean, std) of the advantages as the device computed them, float64.  Synchronises the device: logging and tests."""
        out = (C.c_double * 2)()
        with self._on_device():
            N.check(self._L.crl_rollout_stats(self._h, out))
        return out[0], out[1]

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
        total = self.num_steps * self.num_envs
        size = total // int(num_mini_batch)
        assert size >= 1, f"{total} samples cannot fill {num_mini_batch} minibatches"
        perm = torch.randperm(total, device=self.device, generator=generator)
        for k in range(int(num_mini_batch)):
            yield self.gather(perm[k * size:(k + 1) * size], obs_dtype=obs_dtype)
