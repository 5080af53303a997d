"""A FrameStackTensor bound to the HIP Pong env (frame_stack.py) against everything that can rewrite the env's plane history or the
stack behind the binding's back.  Twin envs with the same seed and the same actions: stack A is bound (``envs.step`` draws it, ``update``
swaps a pointer), stack B stays on the generic kernel, and B is checked against a host numpy restatement of the reference's update
(utils/utils.py:158-170: mask multiply, roll, append) so the comparison does not lean on csrc/frame_stack.hip.  Tolerance 0: stacks are bytes.

The random sequences draw operations from the whole alphabet -- step_envs, forced episode ends, set_state / load_state_dict of a
checkpoint taken earlier, env and stack resets, foreign observations, skipped observations, unbind / bind, masks of the caller's own, and
the device step (with the observation in the env's buffer, in the caller's, or not drawn at all).  The directed tests below them pin one
defect each that the scripted sequences of tests/test_hip_stack_fused.py let through."""
import io

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _twins(n, R, obs_dtype, seed=11):
    import competitive_rl_amd as crl

    mk = lambda: crl.make_envs("cPongDouble-v0", num_envs=n, log_dir=None, seed=seed, resized_dim=R, frame_stack=None, obs_dtype=obs_dtype)
    return mk(), mk()


def _near_the_end(env, which):
    st = env.get_state()
    st["num_rounds"][which] = 20
    env.set_state(st)


def _checkpoint(env):
    buf = io.BytesIO()
    torch.save(env.state_dict(), buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


class HostRef:
    """The reference's FrameStackTensor.update in numpy (float32; a uint8 stack holds the same values)."""

    def __init__(self, n, k, R):
        self.buf = np.zeros((n, k, R, R), np.float32)

    def reset(self):
        self.buf[:] = 0

    def update(self, obs, mask=None):
        if mask is not None:
            self.buf = self.buf * mask.reshape(-1).float().cpu().numpy().reshape(-1, 1, 1, 1)
        self.buf = np.roll(self.buf, -1, axis=1)
        self.buf[:, -1:] = obs.float().cpu().numpy()

    def same(self, fst):
        return np.array_equal(fst.get().float().cpu().numpy(), self.buf)


class Held:
    """What get() / update() hand out stays byte-identical through the next update; the first env call or update after that one may
    recycle the buffer (frame_stack.py: the lifetime of the returned tensor)."""

    def __init__(self):
        self.items = []

    def hand_out(self, t):
        self.items.append([t, t.clone(), 0])

    def before_env_or_update(self):
        self.items = [it for it in self.items if it[2] < 1]

    def before_stack_reset(self, current):
        self.items = [it for it in self.items if it[0].data_ptr() != current.data_ptr()]  # (zeroed by reset(), as the reference's)

    def updated(self):
        for it in self.items:
            it[2] += 1

    def check(self, where):
        for t, copy, age in self.items:
            assert torch.equal(t, copy), ("held tensor changed", where, age)


class Books:
    def __init__(self, n, dev):
        self.ep, self.rr, self.lr, self.steps, self.episodes = torch.zeros((n, 2), dtype=torch.float32, device=dev), [], [], 0, 0

    def step_envs(self, crl, env, fst, acts, dev):
        out = crl.step_envs(acts, env, self.ep, fst, self.rr, self.lr, self.steps, self.episodes, dev, False)
        self.episodes, self.steps = out[5], out[6]
        return out


OPS = (["step"] * 5 + ["step_ends", "run", "run", "run", "set_state", "checkpoint", "env_reset", "stack_reset", "foreign", "skip", "rebind",
                       "own_mask", "dev_step", "dev_no_render", "dev_obs_out"])
ENV_OPS = {"step", "step_ends", "env_reset", "foreign", "skip", "own_mask", "dev_step", "dev_no_render", "dev_obs_out"}  # (or an update)


@pytest.mark.parametrize("obs_dtype,stack_dtype", [("uint8", torch.float32), ("uint8", torch.uint8), ("float32", torch.float32),
                                                   ("float32_ref", torch.float32)])
@pytest.mark.parametrize("R,k", [(84, 4), (42, 4), (84, 2), (42, 1)])
def test_random_operation_sequences_bound_against_generic_and_host(R, k, obs_dtype, stack_dtype):
    """150 operations, 64 envs; after EVERY one: (a) the bound stack equals the generic twin byte for byte (and, every third operation, the
    twin equals the host restatement); (b) every tensor the bound stack handed out is intact through the next update; (c) env A's newest
    observation is untouched by the stack -- which matters where the stack's newest plane IS that observation (frame_stack 1 envs and a
    stack of the env's element type: uint8/uint8, float32/float32).  And the fast path stays: k + 1 plain steps in a row on a bound stack
    end in a pointer swap."""
    _need_gpu()
    import competitive_rl_amd as crl

    n, ops = 64, 150
    a, b = _twins(n, R, obs_dtype, seed=31 + k)
    dev = a.device
    fa = crl.FrameStackTensor(n, (1, R, R), k, dev, dtype=stack_dtype)
    fb = crl.FrameStackTensor(n, (1, R, R), k, dev)
    fb._bind_tried = True                                   # the twin stays on the generic kernel
    ref, held, ba, bb = HostRef(n, k, R), Held(), Books(n, dev), Books(n, dev)
    rs = np.random.RandomState(R + k)
    acts = lambda: torch.as_tensor(rs.randint(0, 3, (n, 2)).astype(np.int32)).to(dev)  # noqa: E731
    assert fa.bind(a)
    oa, ob = a.reset(), b.reset()
    fa.update(oa[0]), fb.update(ob[0]), ref.update(ob[0])
    held.updated()
    snaps = [(a.get_state(), _checkpoint(a))]
    env_copy = a._latest_learner_obs().clone()
    queue, plain_run, long_runs, seen = [], 0, 0, set()

    def both_update(oa_, ob_, mask=None):
        ra = fa.update(oa_, mask)
        fb.update(ob_, mask)
        ref.update(ob_, mask)
        assert ra is fa.get()
        held.updated()

    for t in range(ops):
        if not queue:
            op = OPS[rs.randint(len(OPS))]
            seen.add(op)
            queue = ["step"] * (k + 2) if op == "run" else [op]
        op = queue.pop()
        fused_before = fa.fused_updates
        plain_run = plain_run + 1 if op == "step" else 0
        if op in ENV_OPS:
            held.before_env_or_update()
        if op in ("step", "step_ends"):
            if op == "step_ends":
                which = np.flatnonzero(rs.random_sample(n) < 0.4)
                _near_the_end(a, which), _near_the_end(b, which)
            x = acts()
            oa = ba.step_envs(crl, a, fa, x, dev)
            ob = bb.step_envs(crl, b, fb, x, dev)
            env_copy = a._latest_learner_obs().clone()
            assert torch.equal(oa[2], ob[2]) and torch.equal(oa[4], ob[4]) and ba.episodes == bb.episodes, (t, op)
            assert torch.equal(oa[0][0], ob[0][0]) and torch.equal(oa[0][1], ob[0][1]), (t, op)
            ref.update(ob[0][0], ob[4])
            held.updated()
            if rs.random_sample() < 0.25:
                snaps.append((a.get_state(), _checkpoint(a)))
        elif op == "set_state":
            st = snaps[rs.randint(len(snaps))][0]
            a.set_state(st), b.set_state(st)
        elif op == "checkpoint":
            sd = snaps[rs.randint(len(snaps))][1]
            a.load_state_dict(sd), b.load_state_dict(sd)
        elif op == "env_reset":
            oa, ob = a.reset(), b.reset()
            env_copy = a._latest_learner_obs().clone()
            both_update(oa[0], ob[0])
        elif op == "stack_reset":
            held.before_stack_reset(fa.get())
            fa.reset(), fb.reset(), ref.reset()
        elif op == "foreign":
            f = torch.as_tensor(rs.randint(0, 256, (n, 1, R, R)).astype(np.uint8)).to(dev)
            both_update(f, f)
        elif op in ("skip", "own_mask"):
            x = acts()
            oa, ob = a.step(x), b.step(x)
            env_copy = a._latest_learner_obs().clone()
            if op == "own_mask":
                m = torch.as_tensor((rs.random_sample((n, 1)) < 0.7).astype(np.float32)).to(dev)
                both_update(oa[0][0], ob[0][0], m)
        elif op == "rebind":
            if fa._env is not None:
                fa.unbind()
            assert fa.bind(a)
        elif op == "dev_no_render":
            x = acts()
            a.step_device(x, render=False), b.step_device(x, render=False)
            env_copy = None
        elif op in ("dev_step", "dev_obs_out"):
            x = acts()
            if op == "dev_step":
                bufa, _, _ = a.step_device(x)
                bufb, _, _ = b.step_device(x)
            else:
                bufa, bufb = torch.empty_like(a._obs[0]), torch.empty_like(b._obs[0])
                a.step_device(x, obs_out=bufa), b.step_device(x, obs_out=bufb)
            assert torch.equal(bufa, bufb), (t, op)
            env_copy = a._latest_learner_obs().clone()
            assert fa.update_from_env(a) is fa.get()
            fb.update_from_env(b)
            ref.update(b._latest_learner_obs(), (b._done == 0))
            held.updated()
        held.hand_out(fa.get())
        assert torch.equal(fa.get().float(), fb.get()), ("bound != generic", t, op)                       # (a)
        if t % 3 == 0:
            assert ref.same(fb), ("generic != host restatement", t, op)
        held.check((t, op))                                                                               # (b)
        mine = a._learner_obs
        assert (env_copy is None and mine is None) or torch.equal(mine, env_copy), ("env observation changed", t, op)   # (c)
        if op == "step" and plain_run >= k + 1 and fa._env is not None:
            assert fa.fused_updates == fused_before + 1, ("no pointer swap after a plain stretch", t, plain_run)
            long_runs += 1
    assert ref.same(fb)
    assert long_runs >= 2 and fa.fused_updates >= 10, (seen, long_runs, fa.fused_updates)
    a.close(), b.close()


# ---------------------------------------------------------------------------------------------------- directed: one defect each

@pytest.mark.parametrize("how", ["set_state", "load_state_dict"])
def test_loading_a_state_under_a_bound_stack_keeps_the_trainers_planes(how):
    """A trainer resumes a live env from a checkpoint: the loaded plane history does not explain the trainer's tensor, whose older planes
    are its own -- the update after the load is the generic one, the binding returns once the pre-load planes have rolled out (k generic
    updates at most), and from then on every update is a pointer swap again.  A stack that was reset() follows any history: no fallback."""
    _need_gpu()
    import competitive_rl_amd as crl

    n, R, k = 64, 84, 4
    a, b = _twins(n, R, "uint8", seed=5)
    dev = a.device
    fa, fb = crl.FrameStackTensor(n, (1, R, R), k, dev), crl.FrameStackTensor(n, (1, R, R), k, dev)
    fb._bind_tried = True
    ba, bb = Books(n, dev), Books(n, dev)
    rs = np.random.RandomState(1)
    fa.update(a.reset()[0]), fb.update(b.reset()[0])

    def step():
        x = torch.as_tensor(rs.randint(0, 3, (n, 2)).astype(np.int32)).to(dev)
        ba.step_envs(crl, a, fa, x, dev), bb.step_envs(crl, b, fb, x, dev)

    for _ in range(5):
        step()
    sd = _checkpoint(a)
    for _ in range(10):
        step()
    assert fa.fused_updates == 15
    (a.set_state(sd["env_state"]), b.set_state(sd["env_state"])) if how == "set_state" else (a.load_state_dict(sd), b.load_state_dict(sd))
    generic = 0
    for t in range(12):
        before = fa.fused_updates
        step()
        assert torch.equal(fa.get(), fb.get()), (how, "after the load", t)
        generic += fa.fused_updates == before
    assert 1 <= generic <= k, generic                                      # generic until the pre-load planes are gone ...
    before = fa.fused_updates
    for _ in range(6):
        step()
    assert fa.fused_updates == before + 6                                  # ... then pointer swaps again
    fa.reset(), fb.reset()
    a.load_state_dict(sd), b.load_state_dict(sd)
    before = fa.fused_updates
    for t in range(6):
        step()
        assert torch.equal(fa.get(), fb.get()), (how, "reset stack", t)
    assert fa.fused_updates == before + 6
    a.close(), b.close()


def test_the_re_check_leaves_the_tensor_the_update_before_handed_out():
    """A generic update on a bound stack (here: a foreign observation, then the env's) re-checks the binding against the env's history;
    the tensor the update before it handed out must still be intact when it returns (frame_stack.py: the lifetime of the returned tensor)."""
    _need_gpu()
    import competitive_rl_amd as crl

    n, R, k = 32, 84, 4
    a, b = _twins(n, R, "uint8", seed=6)
    dev = a.device
    fa, fb = crl.FrameStackTensor(n, (1, R, R), k, dev), crl.FrameStackTensor(n, (1, R, R), k, dev)
    fb._bind_tried = True
    ba, bb = Books(n, dev), Books(n, dev)
    rs = np.random.RandomState(2)
    fa.update(a.reset()[0]), fb.update(b.reset()[0])
    step = lambda x: (ba.step_envs(crl, a, fa, x, dev), bb.step_envs(crl, b, fb, x, dev))  # noqa: E731
    acts = lambda: torch.as_tensor(rs.randint(0, 3, (n, 2)).astype(np.int32)).to(dev)  # noqa: E731
    for _ in range(3):
        step(acts())
    foreign = torch.full((n, 1, R, R), 9, dtype=torch.uint8, device=dev)
    for t in range(k + 2):
        held = fa.update(foreign) if t == 0 else fa.get()
        fb.update(foreign) if t == 0 else None
        copy = held.clone()
        step(acts())
        assert torch.equal(held, copy), ("the tensor the update before handed out was overwritten", t)
        assert torch.equal(fa.get(), fb.get()), t
    # a used stack bound afresh: nothing is drawn into the held tensor until the env steps
    fa.unbind()
    held = fa.update(foreign)
    fb.update(foreign)
    held2 = fa.update(foreign)
    fb.update(foreign)
    copy = held.clone()
    assert fa.bind(a)
    assert torch.equal(held, copy) and held2.data_ptr() != held.data_ptr()
    a.close(), b.close()


@pytest.mark.parametrize("obs_dtype,stack_dtype", [("uint8", torch.uint8), ("float32", torch.float32)])
def test_stack_reset_leaves_the_env_observation_alone(obs_dtype, stack_dtype):
    """frame_stack 1 env, stack of the env's element type: the stack's newest plane IS agent 0's observation.  reset() gives the stack
    zeros of its own; the observation the env handed out (and holds as its newest) is untouched, as in the reference."""
    _need_gpu()
    import competitive_rl_amd as crl

    n, R, k = 32, 84, 4
    a, b = _twins(n, R, obs_dtype, seed=8)
    dev = a.device
    fa, fb = crl.FrameStackTensor(n, (1, R, R), k, dev, dtype=stack_dtype), crl.FrameStackTensor(n, (1, R, R), k, dev)
    fb._bind_tried = True
    ba, bb = Books(n, dev), Books(n, dev)
    rs = np.random.RandomState(3)
    fa.update(a.reset()[0]), fb.update(b.reset()[0])
    for _ in range(4):
        x = torch.as_tensor(rs.randint(0, 3, (n, 2)).astype(np.int32)).to(dev)
        oa = ba.step_envs(crl, a, fa, x, dev)
        bb.step_envs(crl, b, fb, x, dev)
    obs = oa[0][0]
    assert obs.untyped_storage().data_ptr() == fa.get().untyped_storage().data_ptr()   # (the aliasing this test is about)
    copy = obs.clone()
    assert copy.any()
    fa.reset(), fb.reset()
    assert torch.equal(obs, copy), "reset() zeroed the env's observation"
    assert torch.equal(a._latest_learner_obs(), copy) and not fa.get().any()
    before = fa.fused_updates
    for t in range(6):
        x = torch.as_tensor(rs.randint(0, 3, (n, 2)).astype(np.int32)).to(dev)
        ba.step_envs(crl, a, fa, x, dev), bb.step_envs(crl, b, fb, x, dev)
        assert torch.equal(fa.get().float(), fb.get()), t
    assert fa.fused_updates == before + 6
    a.close(), b.close()


def _time_limit(crl):
    class TimeLimit(crl.VecEnvWrapper):
        """Ends every env's episode (for the caller) after `limit` steps and passes the observation through unchanged; the env below plays
        on.  `cap`: the loop driving it must have stopped by then."""

        def __init__(self, venv, limit, cap=10 ** 9):
            crl.VecEnvWrapper.__init__(self, venv)
            self.limit, self.cap, self.calls = limit, cap, 0
            self.t = torch.zeros(venv.num_envs, dtype=torch.int64, device=venv.device)

        def reset(self):
            self.t.zero_()
            return self.venv.reset()

        def step_wait(self):
            self.calls += 1
            assert self.calls <= self.cap, "the loop did not see the wrapper's episode ends"
            obs, rew, done, info = self.venv.step_wait()
            self.t += 1
            cut = self.t >= self.limit
            done = done | (cut[:, None] if done.dim() == 2 else cut)
            self.t.masked_fill_(cut, 0)
            return obs, rew, done, info

    return TimeLimit


def test_a_wrapper_that_ends_episodes_is_followed_by_step_envs_and_the_match_loop():
    """A user's VecEnvWrapper whose step_wait truncates episodes: the recorders, total_episodes, the masks and the stack follow the
    wrapper's done, not the flags of the env below (which the wrapper's attribute forwarding would reach).  The tournament wrapper keeps
    the fused path."""
    _need_gpu()
    import competitive_rl_amd as crl

    n, R, k, limit = 48, 42, 4, 3
    TimeLimit = _time_limit(crl)
    env = crl.make_envs("cPongDouble-v0", num_envs=n, log_dir=None, seed=9, resized_dim=R, frame_stack=None)
    w = TimeLimit(env, limit)
    dev = env.device
    f = crl.FrameStackTensor(n, (1, R, R), k, dev)
    ref, books = HostRef(n, k, R), Books(n, dev)
    o = w.reset()
    f.update(o[0]), ref.update(o[0])
    rs = np.random.RandomState(4)
    ends = 0
    for t in range(2 * limit + 1):
        x = torch.as_tensor(rs.randint(0, 3, (n, 2)).astype(np.int32)).to(dev)
        obs, _, ended, _, masks, _, _, _ = books.step_envs(crl, w, f, x, dev)
        want = ((t + 1) % limit == 0)
        assert (bool(ended.all()) and not masks.any()) if want else (not ended.any() and bool(masks.all())), t
        ref.update(obs[0], masks)
        assert ref.same(f), ("stack", t)
        ends += n if want else 0
    assert books.episodes == ends == 2 * n and len(books.rr) == ends, (books.episodes, ends, len(books.rr))
    # the two-policy match loop scores the wrapper's episodes
    w2 = TimeLimit(env, limit, cap=limit)
    rule = lambda obs: [crl.CHEAT_CODES] * n  # noqa: E731
    r0, r1 = crl.evaluate_two_policies_in_batch(rule, rule, w2, n)
    assert sum(r0[:3]) == n and sum(r1[:3]) == n and w2.calls == limit, (r0, r1, w2.calls)
    env.close()
    # the tournament wrapper opts in (its own done_host / _stack_env): still the pointer swap
    tw = crl.make_envs("cPongTournament-v0", num_envs=n, log_dir=None, seed=2)
    dev = tw.env.device
    f1 = crl.FrameStackTensor(n, (1, 42, 42), 4, dev)
    b1 = dict(ep=torch.zeros((n, 1), dtype=torch.float32, device=dev), rr=[], lr=[])
    f1.update(tw.reset())
    for t in range(5):
        x = torch.as_tensor(rs.randint(0, 3, (n,)).astype(np.int32)).to(dev)
        crl.step_envs(x, tw, b1["ep"], f1, b1["rr"], b1["lr"], 0, 0, dev, False)
    assert f1.fused_updates == 5
    tw.close()
