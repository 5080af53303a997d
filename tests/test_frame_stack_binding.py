"""Host logic of a FrameStackTensor bound to an env (competitive_rl_amd/frame_stack.py), on the CPU: WHEN the stack state an env drew
ahead may replace the reference's update (utils/utils.py:158-170) and when the generic update has to run -- against a plain numpy
restatement of that update, with a small fake env that keeps FrameStackTensor's history rule the way the HIP Pong context does (the
descriptors of the last four planes, erased when an episode ends).  The GPU tests (tests/test_hip_stack_fused.py) run the same
situations through the real env and kernels; this file needs neither."""
import numpy as np
import pytest
import torch

from competitive_rl_amd.frame_stack import FrameStackTensor


class FakeRingEnv:
    """What frame_stack.py uses of HipPongVecEnv, over synthetic one-plane observations: step() / reset() keep the last four planes per
    env (None = erased), draw a bound stack's next state into the buffer it offers, and hand out the newest plane as the observation.
    get_state() / set_state() replace the planes behind the stack's back (and move the history epoch, as the HIP env's set_state does).
    ``alias=True``: float32 observations, and a drawn stack's newest plane IS the observation handed out (HipPongVecEnv._stack_alias)."""

    def __init__(self, n, shape=(1, 6, 6), seed=0, alias=False):
        self.n, self.shape, self.rs, self.alias = n, shape, np.random.RandomState(seed), alias
        self.device, self.closed = torch.device("cpu"), False
        self._bound_stack = None
        self._serial, self._last_kind, self._learner, self._hist_epoch = 0, None, None, 0
        self.ring = [[None] * 4 for _ in range(n)]
        self._done = torch.zeros(n, dtype=torch.uint8)
        self.draws = 0

    # ---- the hooks
    def _stack_env(self):
        return self

    def _can_draw_stack(self, fst):
        return fst.num_envs == self.n and fst.num_channels == 1 and fst.frame_stack <= 4 and fst.plane_shape == self.shape[1:] and fst.device == self.device

    def _stack_alias(self, fst):
        return self.alias and fst.dtype == torch.float32

    def _obs_lives_in(self, buf):
        return self._learner is not None and self._learner.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()

    def _is_latest_learner_obs(self, obs):
        return self._learner is not None and isinstance(obs, torch.Tensor) and obs.data_ptr() == self._learner.data_ptr() and obs.shape == self._learner.shape

    def _latest_learner_obs(self):
        return self._learner

    def _paint(self, buf, k, valid):
        """planes oldest to newest = ring planes 4 - k .. 3; planes older than `valid` updates are zeros"""
        self.draws += 1
        buf.zero_()
        for i in range(self.n):
            for j in range(k):
                pl = self.ring[i][4 - k + j]
                if pl is not None and j >= k - valid:
                    buf[i, j] = torch.from_numpy(pl[0].astype(np.float32))

    def _draw_stack_into(self, desc):
        # (the descriptor carries the buffer's address, as it does for the library: a host tensor's memory, here)
        import ctypes as C

        count = self.n * desc.planes * int(np.prod(self.shape[1:]))
        flat = np.ctypeslib.as_array((C.c_float * count).from_address(desc.stack_dev))
        buf = torch.from_numpy(flat).view(self.n, desc.planes, *self.shape[1:])
        self._paint(buf, desc.planes, desc.valid_planes)

    def _advance(self, kind, done):
        fst = self._bound_stack() if self._bound_stack is not None else None
        pre = fst._predraw(self, kind) if fst is not None else None
        new = self.rs.randint(0, 256, (self.n, *self.shape)).astype(np.uint8)
        for i in range(self.n):
            if kind == "reset" or done[i]:
                self.ring[i] = [None, None, None, new[i]]   # the history is erased, the new episode's first plane is the newest
            else:
                self.ring[i] = self.ring[i][1:] + [new[i]]
        self._serial += 1
        self._last_kind = kind
        self._done = torch.from_numpy(done.astype(np.uint8))
        self._learner = torch.from_numpy(new.astype(np.float32) if self.alias else new.copy())
        if pre is not None:
            buf, desc = pre
            self._paint(buf, desc.planes, desc.valid_planes)
            if desc.alias_newest:
                self._learner = buf[:, desc.planes - 1:desc.planes]
            fst._predrawn(self, buf, kind)
        return self._learner

    def reset(self):
        return self._advance("reset", np.zeros(self.n, bool))

    def step(self, p_done=0.2, done=None):
        if done is None:
            done = self.rs.random_sample(self.n) < p_done
        return self._advance("step", np.asarray(done, bool)), np.asarray(done, bool)

    def get_state(self):
        return [list(r) for r in self.ring]

    def set_state(self, st):
        self.ring = [list(r) for r in st]
        self._hist_epoch += 1


class RefStack:
    """utils/utils.py:145-173 in numpy"""

    def __init__(self, n, shape, k):
        self.c, self.buf = shape[0], np.zeros((n, shape[0] * k, *shape[1:]), np.float32)

    def reset(self):
        self.buf[:] = 0

    def update(self, obs, mask=None):
        if mask is not None:
            self.buf *= np.asarray(mask, np.float32).reshape(-1, 1, 1, 1)
        self.buf = np.roll(self.buf, -self.c, axis=1)
        self.buf[:, -self.c:] = np.asarray(obs, np.float32)


def _pair(n=5, k=4, seed=1):
    env = FakeRingEnv(n, seed=seed)
    fst = FrameStackTensor(n, env.shape, k, "cpu")
    # (a host stack has one buffer for its generic update; the bound path swaps two like the device one)
    return env, fst, RefStack(n, env.shape, k)


def _same(fst, ref):
    return np.array_equal(fst.get().numpy(), ref.buf)


def _step_envs_like(env, fst, ref, p_done=0.2):
    obs, done = env.step(p_done)
    mask = (1.0 - done.astype(np.float32)).reshape(-1, 1, 1, 1)
    fst.update(obs, torch.from_numpy(mask), _from_env=env)     # what step_envs passes
    ref.update(obs.numpy(), mask)
    assert _same(fst, ref)


@pytest.mark.parametrize("k", [1, 2, 4])
def test_the_regular_loop_is_all_pointer_swaps(k):
    env, fst, ref = _pair(k=k)
    assert fst.bind(env) and fst._env() is env
    obs = env.reset()
    fst.update(obs), ref.update(obs.numpy())
    assert _same(fst, ref) and fst.fused_updates == 1
    for _ in range(40):
        _step_envs_like(env, fst, ref)
    assert fst.fused_updates == 41


def test_binding_a_used_stack_checks_it_against_the_history_at_the_next_step():
    """bind() of a used stack draws nothing: its other buffer is the tensor the update before last handed out, still held by the
    caller.  The check (one draw + one comparison) runs at the next env step, whose draw ahead recycles that buffer anyway."""
    env, fst, ref = _pair()
    obs = env.reset()
    held = fst.update(obs)                             # unbound: the generic update
    ref.update(obs.numpy())
    obs, done = env.step(0.0)
    fst.update(obs, torch.ones(5, 1, 1, 1)), ref.update(obs.numpy(), np.ones((5, 1, 1, 1), np.float32))
    assert fst.fused_updates == 0 and not fst._zero and _same(fst, ref)
    copy, draws = held.clone(), env.draws
    assert fst.bind(env) and env.draws == draws and not fst._synced
    assert torch.equal(held, copy)                     # the tensor of the update before last is intact through the bind
    _step_envs_like(env, fst, ref)
    assert env.draws == draws + 2 and fst._synced and fst.fused_updates == 1   # at the step: one draw + one comparison, then the draw ahead
    for _ in range(5):
        _step_envs_like(env, fst, ref)
    assert fst.fused_updates == 6
    # a stack whose content the env's history canNOT explain binds, stays generic, and comes back once the strange planes have rolled out
    env2, fst2, ref2 = _pair(seed=3)
    env2.reset()
    junk = torch.full((5, 1, 6, 6), 9, dtype=torch.uint8)
    fst2.update(junk), ref2.update(junk.numpy())
    assert fst2.bind(env2) and not fst2._synced
    for _ in range(8):
        _step_envs_like(env2, fst2, ref2, p_done=0.0)
    assert fst2._synced and fst2.fused_updates >= 3


def test_stack_reset_keeps_the_binding_and_draws_only_younger_planes():
    env, fst, ref = _pair()
    fst.bind(env)
    obs = env.reset()
    fst.update(obs), ref.update(obs.numpy())
    for _ in range(5):
        _step_envs_like(env, fst, ref, p_done=0.0)
    fst.reset(), ref.reset()
    assert _same(fst, ref) and fst._spare is None
    for i in range(6):
        _step_envs_like(env, fst, ref, p_done=0.0)
        assert not fst.get()[:, :max(0, 3 - i)].any()
    assert fst.fused_updates == 1 + 5 + 6


def test_what_falls_back_to_the_generic_update_and_how_the_binding_returns():
    env, fst, ref = _pair(n=7)
    fst.bind(env)
    obs = env.reset()
    fst.update(obs), ref.update(obs.numpy())
    for _ in range(5):
        _step_envs_like(env, fst, ref)
    # (1) the env is reset under a live stack, first observation pushed without a mask: the reference keeps the old planes
    obs = env.reset()
    before = fst.fused_updates
    fst.update(obs), ref.update(obs.numpy())
    assert _same(fst, ref) and fst.fused_updates == before and not fst._synced
    for _ in range(6):
        _step_envs_like(env, fst, ref, p_done=0.0)
    assert fst._synced and fst.fused_updates >= before + 2
    # (2) two env steps for one update
    env.step(0.0)
    before = fst.fused_updates
    for _ in range(7):
        _step_envs_like(env, fst, ref, p_done=0.0)
    assert fst._synced and fst.fused_updates >= before + 2
    # (3) a step's observation pushed WITHOUT a mask (the reference then erases nothing, the env's history does on a done): generic
    obs, done = env.step(1.0)
    before = fst.fused_updates
    fst.update(obs), ref.update(obs.numpy())
    assert _same(fst, ref) and fst.fused_updates == before
    # (4) a mask of the caller's own: the stack leaves the env
    obs, done = env.step(0.0)
    m = torch.tensor([1, 0, 1, 1, 0, 1, 1], dtype=torch.float32).reshape(-1, 1, 1, 1)
    fst.update(obs, m), ref.update(obs.numpy(), m.numpy())
    assert _same(fst, ref) and fst._env is None and env._bound_stack is None
    draws = env.draws
    for _ in range(3):
        obs, done = env.step(0.3)
        mask = (1.0 - done.astype(np.float32)).reshape(-1, 1, 1, 1)
        fst.update(obs, torch.from_numpy(mask)), ref.update(obs.numpy(), mask)
        assert _same(fst, ref)
    assert env.draws == draws                       # nothing is drawn ahead for a stack that is not bound
    # (5) update_from_env: the loop of one's own
    assert fst.bind(env)
    for _ in range(8):
        obs, done = env.step(0.0)
        fst.update_from_env(env)
        ref.update(obs.numpy(), (1.0 - done.astype(np.float32)).reshape(-1, 1, 1, 1))
        assert _same(fst, ref)
    assert fst._synced and fst.fused_updates > before


@pytest.mark.parametrize("k", [1, 2, 4])
def test_set_state_under_a_bound_stack_falls_back_until_the_loaded_planes_roll_out(k):
    """A set_state rewrites the history behind the stack: the trainer's older planes are its own, so the updates after it are generic until
    the pre-load planes have rolled out (k - 1 of them matter), then every update is a pointer swap again; a reset() stack follows any history."""
    env, fst, ref = _pair(k=k)
    fst.bind(env)
    obs = env.reset()
    fst.update(obs), ref.update(obs.numpy())
    for _ in range(3):
        _step_envs_like(env, fst, ref, p_done=0.0)
    snap = env.get_state()
    for _ in range(5):
        _step_envs_like(env, fst, ref, p_done=0.0)
    env.set_state(snap)
    generic = 0
    for _ in range(k + 3):
        before = fst.fused_updates
        _step_envs_like(env, fst, ref, p_done=0.0)                 # (asserts the reference's bytes)
        generic += fst.fused_updates == before
    assert generic == k - 1 and fst._synced, generic
    fst.reset(), ref.reset()
    env.set_state(snap)
    before = fst.fused_updates
    for _ in range(3):
        _step_envs_like(env, fst, ref, p_done=0.0)
    assert fst.fused_updates == before + 3


def test_one_env_draws_one_stack_and_a_closed_env_lets_go():
    env, f1, r1 = _pair()
    f2 = FrameStackTensor(5, env.shape, 4, "cpu")
    assert f1.bind(env) and f2.bind(env)
    assert f1._env is None and env._bound_stack() is f2          # the second binding replaces the first
    obs = env.reset()
    f1.update(obs), f2.update(obs), r1.update(obs.numpy())
    assert _same(f1, r1) and _same(f2, r1) and f1.fused_updates == 0 and f2.fused_updates == 1
    env.closed = True
    obs, done = env.step(0.0)
    mask = torch.ones(5, 1, 1, 1)
    f2.update(obs, mask, _from_env=env), r1.update(obs.numpy(), mask.numpy())
    assert _same(f2, r1)                                          # (a closed env: the generic update, no exception)
    assert not FrameStackTensor(5, env.shape, 4, "cpu", out_of_place=False).bind(FakeRingEnv(5))
    assert not FrameStackTensor(5, (2, 6, 6), 2, "cpu").bind(FakeRingEnv(5))     # two channels per observation: not what the env's history holds
    assert not FrameStackTensor(5, env.shape, 4, "cpu").bind(object())


class HeldTensors:
    """The lifetime contract of frame_stack.py: a tensor handed out by get() / update() stays byte-identical through the next update;
    the first env call or update after that one may recycle its buffer (the bound path draws the next state at the env step)."""

    def __init__(self):
        self.items = []   # [tensor, copy taken when handed out, updates since]

    def hand_out(self, t):
        self.items.append([t, t.clone(), 0])

    def before_env_or_update(self):
        self.items = [it for it in self.items if it[2] < 1]

    def before_stack_reset(self, current):
        self.items = [it for it in self.items if it[0].data_ptr() != current.data_ptr()]   # (zeroed by reset(), as the reference's)

    def updated(self):
        for it in self.items:
            it[2] += 1

    def check(self, where):
        for t, copy, age in self.items:
            assert torch.equal(t, copy), (where, age)


OPS = ["step"] * 6 + ["step_ends"] * 2 + ["run", "set_state", "env_reset", "stack_reset", "foreign", "skip", "rebind", "own_mask"]


@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("k", [1, 2, 4])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_operation_sequences_against_the_reference_update(seed, k, alias):
    """300 operations drawn from everything a trainer may do between two updates of a bound stack -- the step_envs update, forced episode
    ends, set_state to an earlier snapshot, an env reset pushed without a mask, stack.reset(), a foreign observation, an env step without
    an update, unbind / bind, a mask of the caller's own -- and after EVERY one: (a) the stack is the reference's update sequence, byte for
    byte; (b) every tensor handed out is intact through the next update; (c) the env's newest observation is untouched by the stack.  And
    the fast path stays: k + 1 plain steps in a row on a bound stack end in a pointer swap."""
    n = 6
    env = FakeRingEnv(n, seed=100 + seed, alias=alias)
    fst = FrameStackTensor(n, env.shape, k, "cpu")
    ref = RefStack(n, env.shape, k)
    held = HeldTensors()
    rs = np.random.RandomState(seed)
    assert fst.bind(env)
    held.before_env_or_update()
    obs = env.reset()
    env_copy = obs.clone()
    assert fst.update(obs) is fst.get()
    ref.update(obs.numpy())
    held.updated()
    snaps, plain_run, long_runs, seen = [env.get_state()], 0, 0, set()

    def push(o, mask=None, from_env=None):
        out = fst.update(o, None if mask is None else torch.from_numpy(mask), _from_env=from_env)
        assert out is fst.get()
        ref.update(o.numpy(), mask)
        held.updated()

    queue = []
    for t in range(300):
        if not queue:
            op = OPS[rs.randint(len(OPS))]
            seen.add(op)
            queue = ["step"] * (k + 2) if op == "run" else [op]   # ("run": a stretch of plain steps, long enough for the binding to return)
        op = queue.pop()
        fused_before = fst.fused_updates
        plain_run = plain_run + 1 if op == "step" else 0
        if op in ("step", "step_ends", "env_reset", "foreign", "skip", "own_mask"):
            held.before_env_or_update()
        if op in ("step", "step_ends", "skip", "own_mask"):
            obs, done = env.step(0.15) if op != "step_ends" else env.step(done=rs.random_sample(n) < 0.5)
            env_copy = obs.clone()
            if rs.random_sample() < 0.3:
                snaps.append(env.get_state())
            if op in ("step", "step_ends"):
                push(obs, (1.0 - done.astype(np.float32)).reshape(-1, 1, 1, 1), env)      # what step_envs passes
            elif op == "own_mask":
                push(obs, (rs.random_sample(n) < 0.7).astype(np.float32).reshape(-1, 1, 1, 1))
        elif op == "set_state":
            env.set_state(snaps[rs.randint(len(snaps))])
        elif op == "env_reset":
            obs = env.reset()
            env_copy = obs.clone()
            push(obs)
        elif op == "stack_reset":
            held.before_stack_reset(fst.get())
            fst.reset(), ref.reset()
        elif op == "foreign":
            push(torch.from_numpy(rs.randint(0, 256, (n, *env.shape)).astype(np.uint8)))
        elif op == "rebind":
            if fst._env is None:
                assert fst.bind(env)
            else:
                fst.unbind()
        held.hand_out(fst.get())
        assert _same(fst, ref), (t, op)                                                  # (a)
        held.check((t, op))                                                              # (b)
        assert torch.equal(env._latest_learner_obs(), env_copy), (t, op)                 # (c)
        if op == "step" and plain_run >= k + 1 and fst._env is not None:
            assert fst.fused_updates == fused_before + 1, (t, plain_run)
            long_runs += 1
    assert seen == set(OPS) and fst.fused_updates >= 15 and long_runs >= 5, (seen, fst.fused_updates, long_runs)
