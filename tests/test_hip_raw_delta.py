"""Raw observations drawn by the delta writer (crl_draw_raw_delta: only the chunks that differ from the frame the buffer holds) are
byte-equal to a whole draw of the same descriptors (obs_descriptors -> render_descriptors, i.e. crl_render_frames_dev on the sweep
kernel): at the bench size for hundreds of steps with points, game ends and timeouts inside the window, and across every call
that changes the state or the buffers out of turn."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


def _actions(gen, n, single, dev):
    a = torch.randint(0, 4, (n,) if single else (n, 2), generator=gen, device=dev, dtype=torch.int32)
    return torch.where(a == 3, torch.full_like(a, 999), a)  # 0 / 1 / 2 / 999


def _assert_whole(env, buf, what):
    ref = env.render_descriptors(env.obs_descriptors())
    if not torch.equal(buf, ref):
        bad = (buf != ref).reshape(buf.shape[0], buf.shape[1], -1).any(-1).nonzero()[:4].tolist()
        raise AssertionError(f"{what}: (env, view) {bad} differ from a whole draw")


def test_delta_equals_whole_draw_at_bench_size():
    _need_gpu()
    import competitive_rl_amd as crl

    n, steps = 65536, 320
    env = crl.HipPongVecEnv(n, seed=3, mode="raw")
    try:
        env.reset()
        st = env.get_state()
        near_end = np.arange(0, n, 7)  # one point from the game's end: 20-20 in round 20
        st["score_l"][near_end], st["score_r"][near_end], st["num_rounds"][near_end] = 20, 20, 20
        timeout = np.arange(3, n, 11)  # the round's step limit inside the window
        st["num_steps"][timeout] = 10000 - (timeout % 200)
        env.set_state(st)
        gen = torch.Generator(device="cuda").manual_seed(11)
        dones = 0
        for t in range(steps):
            buf, _, done = env.step_device(_actions(gen, n, False, "cuda"))
            dones += int(done.sum())
            _assert_whole(env, buf, f"step {t}")
        after = env.get_state()
        assert dones > n // 7 // 4, dones  # games ended (and were auto-reset) inside the window
        assert (after["num_rounds"][timeout] > 0).any()
    finally:
        env.close()


@pytest.mark.parametrize("single", [False, True])
def test_delta_equals_whole_draw_across_out_of_turn_calls(single):
    _need_gpu()
    import competitive_rl_amd as crl

    n = 300
    env = crl.HipPongVecEnv(n, seed=5, mode="raw", single_player=single)
    other = crl.HipPongVecEnv(n, seed=9, mode="raw", single_player=single)
    try:
        gen = torch.Generator(device="cuda").manual_seed(2)
        env.reset(), other.reset()
        for _ in range(37):
            other.step_device(_actions(gen, n, single, "cuda"))
        slot = torch.empty(env._obs[0].numel(), dtype=torch.uint8, device="cuda")
        for t in range(160):
            a = _actions(gen, n, single, "cuda")
            k = t % 16
            if k == 3:
                env.reset()
                _assert_whole(env, env._obs[env._flip ^ 1], f"reset at {t}")
                continue
            if k == 5:
                env.load_state_dict(other.state_dict())  # another env's state: every descriptor jumps
            elif k == 7:
                env.set_state(env.get_state()[::-1].copy())
            if k in (8, 9):
                env.step_device(a, render=False)
                continue
            if k == 10:
                out, _, _ = env.step_device(a, obs_out=slot)
                _assert_whole(env, out, f"obs_out at {t}")
                continue
            if k in (11, 13):  # in-place torch writes into handed-out views: the next-but-one step draws into that buffer again
                obs, _, _, _ = env.step(a.cpu().numpy())
                _assert_whole(env, env._obs[env._flip ^ 1], f"step {t}")
                views = obs if isinstance(obs, tuple) else (obs,)
                views[0][7].fill_(3)
                views[-1][:, 100:110].zero_()
                continue
            if t % 2:
                obs, _, _, _ = env.step(a.cpu().numpy())
                buf = env._obs[env._flip ^ 1]
                views = obs if isinstance(obs, tuple) else (obs,)
                assert all(v.data_ptr() == buf[:, i].data_ptr() for i, v in enumerate(views))
            else:
                buf, _, _ = env.step_device(a)
            _assert_whole(env, buf, f"step {t}")
    finally:
        env.close(), other.close()


def test_draw_raw_delta_refuses_what_it_cannot_draw():
    _need_gpu()
    import ctypes as C

    import competitive_rl_amd as crl
    from competitive_rl_amd import _native as N

    L = N.load()
    wrapped = crl.HipPongVecEnv(4, mode="wrapped")
    raw = crl.HipPongVecEnv(4, mode="raw")
    try:
        rec = torch.empty(4, dtype=torch.int64, device="cuda")
        buf = raw._obs[0]
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.crl_draw_raw_delta(wrapped._h, C.c_void_p(wrapped._obs[0].data_ptr()), C.c_void_p(rec.data_ptr()), 0, st) == -4
        assert L.crl_draw_raw_delta(raw._h, None, C.c_void_p(rec.data_ptr()), 0, st) == -1
        assert L.crl_draw_raw_delta(raw._h, C.c_void_p(buf.data_ptr()), None, 0, st) == -1
        assert L.crl_draw_raw_delta(raw._h, C.c_void_p(buf.data_ptr() + 8), C.c_void_p(rec.data_ptr()), 0, st) == -1
        assert L.crl_draw_raw_delta(raw._h, C.c_void_p(buf.data_ptr()), C.c_void_p(rec.data_ptr() + 4), 1, st) == -1
        raw.reset()
        assert L.crl_draw_raw_delta(raw._h, C.c_void_p(buf.data_ptr()), C.c_void_p(rec.data_ptr()), 0, st) == 0
        _assert_whole(raw, buf, "whole draw")
        assert torch.equal(rec, raw.obs_descriptors()[6])
    finally:
        wrapped.close(), raw.close()
