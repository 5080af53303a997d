"""A learner's PPO update on the device: ``LightPPO`` for the LightActorCritic (include/crl.h "ppo update", csrc/pong_ppo.hip) and
``FullPPO`` for the full-size ActorCritic ("ppo update, full size", csrc/pong_ppo_full.hip), one interface.

Closes the loop that ``Policy.act_rollout`` and ``RolloutStorage`` open: the gradient of the clipped-surrogate loss is computed straight
from the storage's uint8 planes -- no float32 stack is ever materialised --, Adam steps the learner's master weights in place, and the
new weights go into a served ``Policy`` or a league / arena slot by a device-to-device copy:

    learner = LightPPO("checkpoint.npz", lr=2.5e-4)          # the weights need a critic
    ...                                                       # a rollout as in rollout.py, storage.finish(...)
    learner.update(storage, num_epochs=4, num_mini_batch=32)  # randperm, then grad + step per minibatch; nothing synchronises
    learner.push(policy)                                      # the act calls enqueued after this use the new weights
    learner.push(league, "learner")                           # ... and so does the pool's slot
    print(learner.stats())                                    # (synchronises)

``FullPPO(weights_or_checkpoint, scratch_rows=None, ...)`` is the same for ``Policy(use_light_model=False)`` and a pool's full-size slots;
a minibatch runs in chunks of ``scratch_rows`` samples (17.6 KB of device scratch each, 16 384 by default).

Teacher targets (include/crl.h "ppo update, teacher targets") add ``coef * CE(teacher, learner)`` to either learner's loss.
Distilling a full-size agent into a light one -- the student acts and is recorded, the teacher sees the same frames and resets:

    student, teacher = Policy(light_ckpt, n), Policy(full_ckpt, n, use_light_model=False)
    logits = torch.empty((T, n, 3), device="cuda")
    for t in range(T):
        values, actions, logp = student.act_rollout(frame, reset)          # as in rollout.py; storage.record(...)
        teacher.act_rollout(frame, reset, want_logits=True)
        logits[t] = teacher.logits()
        ...                                                                # env step, storage.outcome(...)
    storage.finish(...)
    learner.update(storage, 4, 32, teacher=Teacher(logits=logits, temperature=2.0, coef=1.0, policy_term=False))
    print(learner.teacher_stats())                                         # ce, kl, agreement, labelled (synchronises)

Cloning RULE_BASED as a warm start -- the labels are what the cheat code 999 would play in the state the frame shows:

    labels = torch.empty((T, n), dtype=torch.int32, device="cuda")
    for t in range(T):
        envs.rule_labels(seat=0, out=labels[t])                            # before the step that consumes the action
        ...
    learner.update(storage, 4, 32, teacher=Teacher(labels=labels, policy_term=False))

``Teacher(logits=..., coef=0.1)`` with the policy term left on is PPO regularised towards the teacher.

The reference ships no trainer: the loss, its summation shape and the optimiser step are the header's written rule;
``rules.ppo_loss_reference`` / ``rules.ppo_full_loss_reference`` (autograd, float64) and ``rules.adam_reference`` (numpy float32) restate them.  There is no CPU path.
"""
import collections
import ctypes as C

import numpy as np
import torch

from . import _native as N
from . import checkpoint as K
from .checkpoint import BLOB_FLOATS, BLOB_LAYOUT, FULL_BLOB_FLOATS, FULL_BLOB_LAYOUT  # noqa: F401  (the blobs' layouts; re-exported)
from .policy_serving import _CRITIC_KEYS, _FULL_KEYS, _KEYS, _SHAPES, Policy, check_full_weights, critic_of, load_full_weights, load_light_weights
from .rules import (PPO_DEFAULTS, PPO_FULL_KEYS, PPO_KEYS, adam_reference, check_teacher, ppo_full_loss_reference,  # noqa: F401  (re-exported)
                    ppo_full_teacher_loss_reference, ppo_loss_reference, ppo_teacher_loss_reference)

PPOStats = collections.namedtuple("PPOStats", ("policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction", "grad_norm", "steps"))
TeacherStats = collections.namedtuple("TeacherStats", ("ce", "kl", "agreement", "labelled"))


class Teacher:
    """Teacher targets for ``grad`` / ``update`` (include/crl.h "ppo update, teacher targets"): a small value object over the CALLER's
    tensors -- they are not learner state, and the learner keeps no reference beyond the call.  Exactly one of
      logits         float32 (T*N, 3) or (T, N, 3): the teacher's logits of every stored sample, softened by ``temperature``
      labels         int32 (T*N,) or (T, N): an action in 0..2 per sample; any other value = no teacher term for that sample
    and optionally ``value_targets`` float32 (T*N,) or (T, N) in place of the stored returns (a teacher's critic).  All contiguous, on
    the learner's device, row ``t * N + e`` the sample ``storage.gather`` calls so.  The loss per sample becomes
    ``policy_term * policy + coef * CE(q, p) + vf * value - ent * entropy``: ``policy_term=False`` is pure imitation, ``coef=0`` with
    ``policy_term=True`` the plain PPO loss.  A wrong dtype, shape or both / neither of logits and labels raise a ``ValueError`` here;
    the device and the row count are checked against the learner and the storage by ``grad``, before any native call."""

    def __init__(self, logits=None, labels=None, value_targets=None, temperature=1.0, coef=1.0, policy_term=True):
        if (logits is None) == (labels is None):
            raise ValueError("a Teacher has logits or labels, exactly one of the two")
        self.temperature, self.coef, self.policy_term = check_teacher(temperature, coef, policy_term)
        self.logits, self.labels, self.value_targets = logits, labels, value_targets
        rows = set()
        for name, t, dtype, tail in (("logits", logits, torch.float32, (3,)), ("labels", labels, torch.int32, ()),
                                     ("value_targets", value_targets, torch.float32, ())):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dtype:
                raise ValueError(f"Teacher: {name} must be a {dtype} tensor")
            lead = t.shape[:t.dim() - len(tail)]
            if tuple(t.shape[t.dim() - len(tail):]) != tail or len(lead) not in (1, 2) or not t.is_contiguous():
                raise ValueError(f"Teacher: {name} must be contiguous (T*N, ...) or (T, N, ...) with trailing shape {tail}, not {tuple(t.shape)}")
            rows.add(int(np.prod(lead)))
        if len(rows) != 1:
            raise ValueError(f"Teacher: the tensors hold different numbers of samples ({sorted(rows)})")
        self.rows = rows.pop()

    def _tensors(self):
        return [t for t in (self.logits, self.labels, self.value_targets) if t is not None]

    def _native(self, device, total):
        """the crl_ppo_teacher of this teacher for a learner on ``device`` and a storage of ``total`` samples"""
        for t in self._tensors():
            if t.device != device:
                raise ValueError(f"Teacher: a tensor lives on {t.device}, the learner on {device}")
        if self.rows != total:
            raise ValueError(f"Teacher: {self.rows} rows, but the storage holds T * N = {total} samples")
        ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
        return N.CrlPpoTeacher(ptr(self.logits), ptr(self.labels), ptr(self.value_targets), self.rows, self.temperature, self.coef, self.policy_term)


def blob_views(blob):
    """The tensors of a flat blob (a torch tensor or a numpy array) as views, by key: the eight of ``BLOB_LAYOUT`` for ``BLOB_FLOATS``
    floats, the ten of ``FULL_BLOB_LAYOUT`` for ``FULL_BLOB_FLOATS``."""
    layout = FULL_BLOB_LAYOUT if blob.shape[0] == FULL_BLOB_FLOATS else BLOB_LAYOUT
    return {k: blob[o:o + int(np.prod(s))].reshape(s) for k, (o, s) in layout.items()}


def _learner_weights(source):
    """The eight float32 arrays of a dict, a checkpoint path or a light ``Policy``; the critic is required."""
    if isinstance(source, Policy):
        if not source.use_light_model:
            raise ValueError("LightPPO trains the LightActorCritic; the policy serves the full-size network")
        w, critic = source.weights, source.critic
    elif isinstance(source, str):
        w, critic = load_light_weights(source), critic_of(source, True, source)
    else:
        w, critic = {k: np.ascontiguousarray(source[k], np.float32) for k in _KEYS}, critic_of(source, True)
        for k in _KEYS:
            if w[k].shape != _SHAPES[k]:
                raise ValueError(f"weights: {k} has shape {w[k].shape}, LightActorCritic on (4, 42, 42) needs {_SHAPES[k]}")
    if critic is None:
        raise ValueError("a learner needs a critic: critic_w / critic_b beside the weights")
    return {**{k: w[k] for k in _KEYS}, **{k: critic[k] for k in _CRITIC_KEYS}}


def _full_learner_weights(source):
    """The ten float32 arrays of a dict, a checkpoint path or a full-size ``Policy``; the critic is required."""
    if isinstance(source, Policy):
        if source.use_light_model:
            raise ValueError("FullPPO trains the full-size ActorCritic; the policy serves the LightActorCritic")
        w, critic = source.weights, source.critic
    elif isinstance(source, str):
        w, critic = load_full_weights(source), critic_of(source, False, source)
    else:
        if "conv3_w" not in source:
            raise ValueError("FullPPO trains the full-size ActorCritic; the weights have no conv3 (LightPPO trains the LightActorCritic)")
        w, critic = check_full_weights(source), critic_of(source, False)
    if critic is None:
        raise ValueError("a learner needs a critic: critic_w / critic_b beside the weights")
    return {**{k: w[k] for k in _FULL_KEYS}, **{k: critic[k] for k in _CRITIC_KEYS}}


def _plain(hyper):
    return {k: (tuple(x) if isinstance(x, (tuple, list)) else x) for k, x in hyper.items()}


class _PPOLearner:
    """What the learners share (the two of Pong here, ``car_learner.CarPPO``): everything but the network's tensors, its create /
    weight calls, its statistics and its push targets.  A subclass names what differs as class attributes."""
    _C = "crl_ppo_"              # the C prefix of the learner's calls
    _DEFAULTS = PPO_DEFAULTS     # the hyper-parameters and their defaults
    _KEYS, _LAYOUT, _FLOATS = PPO_KEYS, BLOB_LAYOUT, BLOB_FLOATS
    _SIZED = True                # crl_ppo_get_state / set_state carry the blob's size and scratch_rows: one C object, two networks
    _weights_of = staticmethod(_learner_weights)
    _views = staticmethod(blob_views)                                  # a flat blob as the tensors' views by key
    _TEACHER = Teacher           # the value object ``grad(teacher=)`` takes

    def _open(self, device, hyper):
        """What every constructor starts with: the GPU, the hyper-parameters, the device."""
        name = type(self).__name__
        if not torch.cuda.is_available():
            raise RuntimeError(f"competitive_rl_amd.{name} needs a ROCm GPU; there is no CPU fallback")
        unknown = set(hyper) - set(self._DEFAULTS)
        if unknown:
            raise TypeError(f"unknown hyper-parameters {sorted(unknown)}; {name} takes {sorted(self._DEFAULTS)}")
        self.hyper = dict(self._DEFAULTS, **hyper)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())

    def _setup(self, weights_or_checkpoint, device, hyper):
        self._open(device, hyper)
        w = self._weights_of(weights_or_checkpoint)
        self._L = N.load()
        return [w[k].ctypes.data_as(C.c_void_p) for k in self._KEYS]

    def _c(self, name):
        return getattr(self._L, self._C + name)

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _hyper(self):
        h = self.hyper
        return N.CrlPpoHyper(h["clip"], h["vf_coef"], h["ent_coef"], h["lr"], h["betas"][0], h["betas"][1], h["eps"], h["max_grad_norm"])

    def close(self):
        if getattr(self, "_h", None):
            self._c("destroy")(self._h)
            self._h = None

    __del__ = close

    def _dev_blob(self, ptr):
        """A float32 (blob floats,) tensor over the learner's own device memory at ``ptr`` (valid while the learner lives)."""
        iface = {"shape": (self._FLOATS,), "typestr": "<f4", "data": (ptr, False), "version": 2}
        holder = type("_Blob", (), {"__cuda_array_interface__": iface, "_keep": self})()
        return torch.as_tensor(holder, device=self.device)

    def grad(self, storage, idx, teacher=None):
        """The gradient of the loss over the samples ``idx`` (int64 on the device, flat ``t * num_envs + e``, as ``storage.gather`` takes
        them) of a finished ``RolloutStorage``, at the learner's weights: a dict of device VIEWS of the gradient tensors, for
        callers with their own optimiser; the next ``grad`` overwrites them.  ``teacher``: a ``Teacher`` adds its term to the loss
        (``teacher_stats()`` then has its statistics); None is the plain PPO loss.  No synchronisation."""
        assert idx.device == self.device and idx.dtype == torch.int64 and idx.dim() == 1, "idx: int64 (B,) on the learner's device"
        assert storage.device == self.device, "the storage lives on another device"
        idx = idx.contiguous()
        hyper = self._hyper()
        if teacher is not None:
            if not isinstance(teacher, self._TEACHER):
                raise ValueError(f"teacher must be a {self._TEACHER.__name__} or None, not {type(teacher).__name__}")
            native = teacher._native(self.device, storage._total())
        with torch.cuda.device(self.device):
            ip = C.c_void_p(idx.data_ptr()) if idx.numel() else None
            if teacher is None:
                N.check(self._c("grad")(self._h, storage._h, ip, idx.numel(), C.byref(hyper), self._stream()))
            else:
                N.check(self._c("grad_teacher")(self._h, storage._h, ip, idx.numel(), C.byref(hyper), C.byref(native), self._stream()))
                for t in teacher._tensors():  # (the launches read them: a caching allocator must not hand them out before that)
                    t.record_stream(torch.cuda.current_stream(self.device))
            p = C.c_void_p()
            N.check(self._c("get_grad")(self._h, C.byref(p), None))
        return self._views(self._dev_blob(p.value))

    def step(self):
        """Clips the last gradient to ``max_grad_norm`` and takes one Adam step on the master weights, in place.  No synchronisation."""
        hyper = self._hyper()
        with torch.cuda.device(self.device):
            N.check(self._c("step")(self._h, C.byref(hyper), self._stream()))

    def update(self, storage, num_epochs, num_mini_batch, generator=None, teacher=None):
        """``num_epochs`` passes over the finished ``storage``: per pass one ``torch.randperm`` on the device (``generator``: a device
        generator, for a reproducible order) cut into ``num_mini_batch`` batches of T * N // num_mini_batch samples, ``grad`` and ``step``
        per batch; ``teacher`` goes to every ``grad``.  Nothing synchronises."""
        total = storage._total()
        size = total // int(num_mini_batch)
        assert size >= 1, f"{total} samples cannot fill {num_mini_batch} minibatches"
        extra = () if teacher is None else (teacher,)  # (a learner without a teacher term takes none)
        for _ in range(int(num_epochs)):
            perm = torch.randperm(total, device=self.device, generator=generator)
            for k in range(int(num_mini_batch)):
                self.grad(storage, perm[k * size:(k + 1) * size], *extra)
                self.step()

    def teacher_stats(self):
        """``TeacherStats`` of the last ``grad`` with a teacher: the means over the batch of the cross-entropy to the target, of
        KL(teacher || learner), of the samples whose greedy action is the target's, and the share of samples that had a teacher term.
        Refuses after a plain ``grad``.  Synchronises the device: logging and tests."""
        out = (C.c_double * 4)()
        with torch.cuda.device(self.device):
            N.check(self._c("teacher_stats")(self._h, out))
        return TeacherStats(*out)

    def _blob_dev(self, target):
        p = C.c_void_p()
        N.check(self._c("weights_dev")(self._h, C.byref(p)))
        assert target.device == self.device, "the target lives on another device"
        return p

    def weights(self):
        """The master weights as a dict of float32 numpy arrays in torch layout (synchronises)."""
        w = {k: np.zeros(s, np.float32) for k, (_, s) in self._LAYOUT.items()}
        with torch.cuda.device(self.device):
            N.check(self._get(self._h, *[w[k].ctypes.data_as(C.c_void_p) for k in self._KEYS]))
        return w

    def set_weights(self, weights_or_checkpoint):
        """Replaces the master weights and zeroes Adam's moments and step count (synchronises)."""
        w = self._weights_of(weights_or_checkpoint)
        with torch.cuda.device(self.device):
            N.check(self._set(self._h, *[w[k].ctypes.data_as(C.c_void_p) for k in self._KEYS]))

    def stats(self):
        """``PPOStats`` of the last ``grad``: the means of policy loss, value loss, entropy, ``old_logp - logp`` and the clipped share, the
        gradient's norm before clipping, the optimiser steps taken.  Synchronises the device: logging and tests."""
        out = (C.c_double * 7)()
        with torch.cuda.device(self.device):
            N.check(self._L.crl_ppo_stats(self._h, out))
        return PPOStats(*out[:6], int(out[6]))

    # ---- checkpoint / resume (include/crl.h "checkpoint / resume")
    def _state(self, want_blobs=True):
        """(weights blob, m blob, v blob, steps, scratch_rows) as the device holds them, behind the work enqueued on the current stream"""
        blobs = [np.empty(self._FLOATS, np.float32) if want_blobs else None for _ in range(3)]
        steps, rows = C.c_int64(), C.c_int64()
        tail = (self._FLOATS, C.byref(steps), C.byref(rows)) if self._SIZED else (C.byref(steps),)
        with torch.cuda.device(self.device):
            N.check(self._c("get_state")(self._h, *[b.ctypes.data_as(C.c_void_p) if want_blobs else None for b in blobs], *tail, self._stream()))
        return blobs[0], blobs[1], blobs[2], steps.value, rows.value

    def _split(self, blob):
        """A host blob as the dict of arrays by key that ``state_dict`` carries."""
        return K.split_blob(blob, self._LAYOUT)

    def _state_blobs(self, sd):
        """The tensor half of ``load_state_dict``: the three host blobs of ``sd``'s weights, m and v, or a refusal."""
        name = type(self).__name__
        rows = self._state(want_blobs=False)[4]
        if rows and int(sd.get("scratch_rows", -1)) != rows:
            raise K.refuse(f"{name}: scratch_rows is {sd.get('scratch_rows')} in the state dict and {rows} here (it is part of the summation shape)")
        return [K.join_blob(sd.get(k), self._LAYOUT, self._FLOATS, f"{name} {k}") for k in ("weights", "m", "v")]

    def state_dict(self):
        """Everything a continuation needs, as host arrays (SYNCHRONISES with the current stream): ``kind``, the master ``weights`` by
        key, Adam's moments ``m`` and ``v`` by key in the same layout, the optimiser ``steps`` taken, ``hyper`` and, for ``FullPPO``,
        ``scratch_rows`` (part of the summation shape).  The last gradient and its statistics are not state."""
        w, m, v, steps, rows = self._state()
        sd = {"kind": type(self).__name__, "weights": self._split(w), "m": self._split(m), "v": self._split(v), "steps": steps,
              "hyper": _plain(self.hyper)}
        if rows:
            sd["scratch_rows"] = rows
        return sd

    def load_state_dict(self, sd):
        """Puts a ``state_dict()`` back: weights, both moments and the step count together, and ``hyper``.  Everything is looked at
        before anything is written: the other learner's dict, a missing or misshapen tensor, a negative step count, unknown
        hyper-parameters or -- ``FullPPO`` -- another ``scratch_rows`` raise a ``ValueError`` and leave the learner as it was.  Ordered
        on the current stream and SYNCHRONISES with it.  Afterwards the learner has no gradient: ``step()`` / ``stats()`` refuse until
        the next ``grad``, as on a fresh learner."""
        name = type(self).__name__
        K.check_header(sd, name, name)
        blobs = self._state_blobs(sd)
        steps = K.check_counter(sd.get("steps"), 63, "steps", name)
        hyper = sd.get("hyper", self.hyper)
        if not isinstance(hyper, dict) or set(hyper) - set(self._DEFAULTS):
            raise K.refuse(f"{name}: hyper must be a dict with keys of {sorted(self._DEFAULTS)}")
        tail = (self._FLOATS, steps) if self._SIZED else (steps,)
        with torch.cuda.device(self.device):
            N.check(self._c("set_state")(self._h, *[b.ctypes.data_as(C.c_void_p) for b in blobs], *tail, self._stream()))
        self.hyper = dict(self._DEFAULTS, **_plain(hyper))


class LightPPO(_PPOLearner):
    def __init__(self, weights_or_checkpoint, device=None, **hyper):
        """``weights_or_checkpoint``: a dict of the eight arrays in torch layout (``rules.PPO_KEYS``), an ``.npz`` or reference checkpoint
        that carries a critic, or a light ``Policy`` with one.  ``hyper``: ``clip``, ``vf_coef``, ``ent_coef``, ``lr``, ``betas``, ``eps``,
        ``max_grad_norm`` (``rules.PPO_DEFAULTS``); attributes of the same names may be changed between calls."""
        ptr = self._setup(weights_or_checkpoint, device, hyper)
        self._get, self._set = self._L.crl_ppo_get_weights, self._L.crl_ppo_set_weights
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._L.crl_ppo_create(self.device.index or 0, *ptr, C.byref(h)))
        self._h = h

    def push(self, target, name=None):
        """The master weights into a served light ``Policy`` (its critic too), or into slot ``name`` (a name or an index) of a
        ``LeagueEnvWrapper`` / ``LeagueArena``: one device-to-device copy ordered on the current stream, the host is not touched.  The
        target's host-side copy of its weights (``Policy.weights``) is NOT refreshed: ``weights()`` has the learner's."""
        p = self._blob_dev(target)
        with torch.cuda.device(self.device):
            if isinstance(target, Policy):
                N.check(self._L.crl_policy_load_weights_dev(target._h, p, self._stream()))
            else:
                N.check(self._L.crl_pool_load_light_dev(target._h, target._agent_index(name), p, self._stream()))


class FullPPO(_PPOLearner):
    _KEYS, _LAYOUT, _FLOATS = PPO_FULL_KEYS, FULL_BLOB_LAYOUT, FULL_BLOB_FLOATS
    _weights_of = staticmethod(_full_learner_weights)

    def __init__(self, weights_or_checkpoint, device=None, scratch_rows=None, **hyper):
        """``weights_or_checkpoint``: a dict of the ten arrays in torch layout (``rules.PPO_FULL_KEYS``), an ``.npz`` or reference
        checkpoint with ``critic_linear.*``, or a full-size ``Policy`` with a critic.  ``scratch_rows``: samples per chunk of a
        minibatch (17.6 KB of device scratch each; default 16 384, at least 64) -- part of the summation shape, so two learners give the same bits
        only with the same value.  ``hyper`` as for ``LightPPO``."""
        ptr = self._setup(weights_or_checkpoint, device, hyper)
        self._get, self._set = self._L.crl_ppo_get_weights_full, self._L.crl_ppo_set_weights_full
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            N.check(self._L.crl_ppo_create_full(self.device.index or 0, int(scratch_rows or 0), *ptr, C.byref(h)))
        self._h = h

    def push(self, target, name=None):
        """The master weights into a served full-size ``Policy`` (its critic too), or into full-size slot ``name`` (a name or an index)
        of a ``LeagueEnvWrapper`` / ``LeagueArena``: one device-to-device copy ordered on the current stream, the host is not touched.
        A light ``Policy`` or slot is refused.  The target's host-side copy of its weights is NOT refreshed: ``weights()`` has them."""
        p = self._blob_dev(target)
        with torch.cuda.device(self.device):
            if isinstance(target, Policy):
                N.check(self._L.crl_policy_load_full_dev(target._h, p, self._stream()))
            else:
                N.check(self._L.crl_pool_load_full_dev(target._h, target._agent_index(name), p, self._stream()))
