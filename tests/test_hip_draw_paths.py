"""GPU tests of the one Pong draw path and the one step routine on the host side: the observation a step returns, the same step
drawn into a caller's tensor, the frames re-drawn from their descriptors and the terminal observations all go through one
launch routine of the library and one step routine of HipPongVecEnv, and must stay byte-equal (every comparison is torch.equal)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N_ENVS, STEPS = 5, 40
# env -> wrapped step on which its episode ends: the ball leaves on the left on frame 3 of that step (x = 13 + 16 s: four
# frames of 4 px per step, out at x < 0), so no frame of the step is skipped and both kept frames are the step's own
FINISH = {1: 0, 3: 2}
WRAPPED = [(R, K, dt) for (R, K) in ((84, 1), (84, 4), (42, 4)) for dt in ("uint8", "float32", "float32_ref")]
CASES = [("wrapped", R, K, dt, single) for (R, K, dt) in WRAPPED for single in (False, True)] + [("raw", 84, 1, "uint8", s) for s in (False, True)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _make(mode, R, K, dt, single, seed=11):
    import competitive_rl_amd as crl
    env = crl.HipPongVecEnv(N_ENVS, seed=seed, mode=mode, resized_dim=R, frame_stack=K, obs_dtype=dt, single_player=single)
    env.reset()
    return env


def _near_end(env, rounds):
    """Envs of FINISH one lost ball away from their step, with `rounds` rounds played (20 = the ball ends the episode); the left
    bat parked at the bottom, out of the ball's way whatever the actions."""
    st = env.get_state()
    for i, s in FINISH.items():
        st["ball_x"][i], st["ball_y"][i], st["speed_x"][i], st["speed_y"][i] = 13 + 16 * s, 40, -4.0, 0.5
        st["bat_l_y"][i], st["num_rounds"][i] = 170, rounds
        st["score_l"][i], st["score_r"][i] = 2 + i, 5
    env.set_state(st)


def _actions(rs, single):
    a = rs.randint(0, 3, (N_ENVS,) if single else (N_ENVS, 2)).astype(np.int32)
    return a, torch.as_tensor(a).cuda()


def _stack(obs, single):
    return obs[:, None] if single else torch.stack(obs, 1)  # (N, V, ...), the layout of the observation buffer


def _views(term, single):
    return term[None] if single else torch.stack(term, 0)  # (V, ...): one env's terminal observation


@pytest.mark.parametrize("mode,R,K,dt,single", CASES)
def test_step_obs_out_descriptors_and_terminal_frames_agree(mode, R, K, dt, single):
    """step()'s observation == the same step drawn into a caller's tensor by a second context == the observation re-drawn from
    its descriptors.  Terminal observations: device and host index lists agree, and equal the frames drawn from the descriptors
    of a third context in which the same ball does NOT end the episode (num_rounds 0 instead of 20: the frames of the step are
    the same, but they stay the current observation instead of being replaced by the restarted episode's)."""
    _need_gpu()
    raw = mode == "raw"
    a, b, c = (_make(mode, R, K, dt, single) for _ in range(3))
    _near_end(a, 20), _near_end(b, 20), _near_end(c, 0)
    slot = torch.empty_like(a._obs[0])
    rs = np.random.RandomState(5)
    finished = set()
    per_step = 4 if raw else 1  # a raw step is one frame: step s of the table is frames 4 s .. 4 s + 3
    for t in range(STEPS):
        host, dev = _actions(rs, single)
        obs, _, done, infos = a.step(host)
        got = _stack(obs, single)
        assert torch.equal(got, a.render_descriptors(a.obs_descriptors())), t
        out, _, bdone = b.step_device(dev, obs_out=slot)
        assert out.data_ptr() == slot.data_ptr() and torch.equal(got, out), t
        c.step_device(dev, render=False)
        flags = done if done.dim() == 1 else done[:, 0]
        assert torch.equal(flags, bdone.bool())
        idx = torch.nonzero(flags).reshape(-1)
        if not idx.numel():
            continue
        by_dev, by_host = a.terminal_observation(idx), a.terminal_observation(idx.cpu().numpy())
        frames = c.render_descriptors(c.obs_descriptors())  # (N, V, 210, 160, 3) | (N, V, K, R, R): the newest plane is the step's
        for k, i in enumerate(idx.cpu().tolist()):
            finished.add(i)
            td, th, ti = (_views(x, single) for x in (by_dev[k], by_host[k], infos[i]["terminal_observation"]))
            assert torch.equal(td, th) and torch.equal(td, ti), (t, i)
            if FINISH.get(i) is not None and t == FINISH[i] * per_step + per_step - 1:
                want = frames[i] if raw else frames[i][:, K - 1:K]
                assert torch.equal(td, want), (t, i)
    assert set(FINISH) <= finished
    for e in (a, b, c):
        e.close()


@pytest.mark.parametrize("mode", ["wrapped", "raw"])
@pytest.mark.parametrize("form", ["step", "step_device", "obs_out"])
def test_refused_step_leaves_the_books_alone(mode, form):
    """An out-of-range device action is reported by the NEXT call, which does no work: the observation buffers, the serial and the
    next step's output equal those of a context that never saw the bad action (the bat of a bad action stays put = action 1)."""
    _need_gpu()
    from competitive_rl_amd._native import CrlActionError
    x, y = (_make(mode, 84, 4, "uint8", False) for _ in range(2))
    slots = [torch.zeros_like(e._obs[0]) for e in (x, y)]
    rs = np.random.RandomState(9)

    def call(env, slot, host, dev):
        if form == "step":
            return _stack(env.step(host)[0], False)
        return env.step_device(dev, obs_out=slot if form == "obs_out" else None)[0]

    host, dev = _actions(rs, False)
    assert torch.equal(call(x, slots[0], host, dev), call(y, slots[1], host, dev))
    bad = dev.clone()
    bad[2, 0], dev[2, 0] = 7, 1
    x.step_device(bad), y.step_device(dev)
    torch.cuda.synchronize()
    before = (x._serial, x._flip, [o.clone() for o in x._obs], slots[0].clone())
    host, dev = _actions(rs, False)
    with pytest.raises(CrlActionError):
        call(x, slots[0], host, dev)
    assert (x._serial, x._flip) == before[:2] == (y._serial, y._flip)
    for k in range(2):
        assert torch.equal(x._obs[k], before[2][k]) and torch.equal(x._obs[k], y._obs[k])
    assert torch.equal(slots[0], before[3]) and torch.equal(slots[0], slots[1])
    assert torch.equal(call(x, slots[0], host, dev), call(y, slots[1], host, dev))  # the report was made once: this call proceeds
    assert x._serial == y._serial and x._flip == y._flip
    assert x.get_state().tobytes() == y.get_state().tobytes()
    x.close(), y.close()
