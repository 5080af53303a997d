"""The one-launch raw step (crl_step_raw_delta: every env stepped and the changed chunks of its observation stored by the wavefront
that stepped it) against the two calls it replaces (crl_step_stack + crl_draw_raw_delta, ``env._fused_raw_step = False``) and against
a whole draw of the same descriptors.  Every comparison is byte equality."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

STEP_W = (8, 16, 32, 64)  # the candidates for the envs a wavefront or a workgroup of the one-launch step owns


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


def _same(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()  # (get_state()'s packed records, every field)


def _twins(n, seed, single):
    import competitive_rl_amd as crl

    fused = crl.HipPongVecEnv(n, seed=seed, mode="raw", single_player=single)
    twin = crl.HipPongVecEnv(n, seed=seed, mode="raw", single_player=single)
    fused._fused_raw_step, twin._fused_raw_step = True, False
    return fused, twin


def _near_end(env, n, every):
    """tests/test_hip_raw_delta.py's state: 20-20 in round 20 for every 7th env (`every`: for all of them), the round's step limit
    inside the window for every 11th"""
    st = env.get_state()
    near_end = np.arange(0, n, 1 if every else 7)
    st["score_l"][near_end], st["score_r"][near_end], st["num_rounds"][near_end] = 20, 20, 20
    timeout = np.arange(3, n, 11)
    st["num_steps"][timeout] = 10000 - (timeout % 200)
    return st


def _warm(envs, gen, n, single, steps=2):
    """reset and the two steps that draw each buffer whole: from the third step on a buffer's record is valid"""
    for e in envs:
        e.reset()
    for _ in range(steps):
        a = _actions(gen, n, single, "cuda")
        for e in envs:
            e.step_device(a)


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 17, 31, 33, 63, 65, 300])
def test_twin_envs(n, single):
    _need_gpu()
    steps = 200
    fused, twin = _twins(n, 3, single)
    try:
        gen = torch.Generator(device="cuda").manual_seed(11)
        _warm((fused, twin), gen, n, single)
        st = _near_end(fused, n, every=n < 63)
        fused.set_state(st), twin.set_state(st)
        fused.kernel_timing(True)
        fused.kernel_time_ms(0), fused.kernel_time_ms(1)
        dones = 0
        for t in range(steps):
            a = _actions(gen, n, single, "cuda")
            bf, rf, df = fused.step_device(a)
            bt, rt, dt = twin.step_device(a)
            assert torch.equal(bf, bt), f"step {t}: the observations of the two envs differ"
            _assert_whole(fused, bf, f"step {t}, one launch")
            _assert_whole(twin, bt, f"step {t}, two launches")
            assert torch.equal(rf, rt) and torch.equal(df, dt), f"step {t}: rewards or dones differ"
            dones += int(df.sum())
        assert dones > 0, "no game ended inside the window"
        torch.cuda.synchronize()
        assert fused.kernel_time_ms(0)[1] == 0, "the one-launch path brackets no dynamics launch"
        assert fused.kernel_time_ms(1)[1] == steps
        sf, stw = fused.get_state(), twin.get_state()
        for k in sf.dtype.names:
            assert np.array_equal(sf[k], stw[k]), k
        for k in range(2):
            assert torch.equal(fused._drawn[k], twin._drawn[k]), f"record {k}"
    finally:
        fused.close(), twin.close()


@pytest.mark.parametrize("single", [False, True])
def test_out_of_turn_calls(single):
    """the sequence of tests/test_hip_raw_delta.py::test_delta_equals_whole_draw_across_out_of_turn_calls, the one-launch path on"""
    _need_gpu()
    import competitive_rl_amd as crl

    n = 300
    env = crl.HipPongVecEnv(n, seed=5, mode="raw", single_player=single)
    other = crl.HipPongVecEnv(n, seed=9, mode="raw", single_player=single)
    try:
        env._fused_raw_step = True
        env.kernel_timing(True)
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
        torch.cuda.synchronize()
        # both routes were in use.  Slot 0 holds the dynamics launches: the 20 undrawn steps and every two-call step; slot 1 the draws:
        # the 10 resets, every two-call step that draws and every one-launch step
        dyn, ras = env.kernel_time_ms(0)[1], env.kernel_time_ms(1)[1]
        one_launch = (ras - 10) - (dyn - 20)
        assert dyn > 20 and one_launch >= 40, (dyn, ras)
    finally:
        env.close(), other.close()


@pytest.mark.parametrize("single", [False, True])
def test_out_of_range_action(single):
    _need_gpu()
    from competitive_rl_amd import _native as N

    n = 40
    fused, twin = _twins(n, 7, single)
    try:
        gen = torch.Generator(device="cuda").manual_seed(5)
        _warm((fused, twin), gen, n, single, steps=3)
        fused.kernel_timing(True)
        before = fused.get_state()
        a = torch.ones((n,) if single else (n, 2), dtype=torch.int32, device="cuda")  # 1: the bat stays
        if single:
            a[2] = 7
        else:
            a[2, 0], a[5, 1] = 7, -3
        for e in (fused, twin):
            e.step_device(a)
        torch.cuda.synchronize()
        assert fused.kernel_time_ms(0)[1] == 0 and fused.kernel_time_ms(1)[1] == 1, "the bad action did not go through the one-launch route"
        after = fused.get_state()
        assert after["bat_l_y"][2] == before["bat_l_y"][2]
        if not single:
            assert after["bat_r_y"][5] == before["bat_r_y"][5]
        assert _same(after, twin.get_state())
        # the next call reports it, once, and does no work
        ok = _actions(gen, n, single, "cuda")
        k = fused._flip
        held, rec = fused._obs[k].clone(), fused._drawn[k].clone()
        with pytest.raises(N.CrlActionError):
            fused.step_device(ok)
        with pytest.raises(N.CrlActionError):
            twin.step_device(ok)
        torch.cuda.synchronize()
        assert fused._flip == k and _same(fused.get_state(), after), "the refused call stepped the envs"
        assert torch.equal(fused._obs[k], held) and torch.equal(fused._drawn[k], rec), "the refused call drew"
        for t in range(4):
            ok = _actions(gen, n, single, "cuda")
            bf, rf, df = fused.step_device(ok)
            bt, rt, dt = twin.step_device(ok)
            assert torch.equal(bf, bt) and torch.equal(rf, rt) and torch.equal(df, dt), f"step {t} after the report"
            _assert_whole(fused, bf, f"step {t} after the report")
        torch.cuda.synchronize()
        assert _same(fused.get_state(), twin.get_state())
    finally:
        fused.close(), twin.close()


def test_done_host():
    _need_gpu()
    n = 70
    fused, twin = _twins(n, 13, False)
    try:
        gen = torch.Generator(device="cuda").manual_seed(17)
        _warm((fused, twin), gen, n, False, steps=3)
        st = _near_end(fused, n, every=True)
        fused.set_state(st), twin.set_state(st)
        fused.kernel_timing(True)
        a = _actions(gen, n, False, "cuda")
        _, _, df = fused.step_device(a)
        twin.step_device(a)
        torch.cuda.synchronize()
        assert fused.kernel_time_ms(0)[1] == 0  # (still one launch)
        assert np.array_equal(fused.done_host(), df.bool().cpu().numpy())  # the first call sets the event: two launches from now on
        steps, dones = 30, 0
        for t in range(steps):
            a = _actions(gen, n, False, "cuda")
            bf, rf, df = fused.step_device(a)
            early = fused.done_host()
            bt, rt, dt = twin.step_device(a)
            assert np.array_equal(early, df.bool().cpu().numpy()), f"step {t}: done_host() is not the step's done flags"
            assert torch.equal(bf, bt) and torch.equal(rf, rt) and torch.equal(df, dt), f"step {t}"
            _assert_whole(fused, bf, f"step {t}")
            dones += int(df.sum())
        assert dones > 0
        torch.cuda.synchronize()
        assert fused.kernel_time_ms(0)[1] == steps, "with a flags event the dynamics launch is its own again"
        assert _same(fused.get_state(), twin.get_state())
    finally:
        fused.close(), twin.close()


@pytest.mark.parametrize("single", [False, True])
@pytest.mark.parametrize("w", STEP_W)
def test_direct_calls_into_a_padded_allocation(w, single):
    """the observation 16 bytes into a 64-byte block (single-chunk stores), n = 2 W + 3, one env's worth of sentinel bytes behind
    every array the call writes"""
    _need_gpu()
    import competitive_rl_amd as crl
    from competitive_rl_amd import _native as N

    n, steps, fill = 2 * w + 3, 60, 0xA5
    env = crl.HipPongVecEnv(n, seed=21, mode="raw", single_player=single)
    try:
        L = N.load()
        env.reset()
        st = _near_end(env, n, every=True)
        env.set_state(st)
        per_env = env._obs[0][0].numel()
        store = torch.full(((n + 1) * per_env + 128,), fill, dtype=torch.uint8, device="cuda")
        off = (-store.data_ptr()) % 64 + 16
        buf = store[off:off + n * per_env].view(env._obs[0].shape)
        assert buf.data_ptr() % 64 == 16
        sentinel = -0x5A5A5A5A5A5A5A5B
        rec = torch.full((n + 1,), sentinel, dtype=torch.int64, device="cuda")
        rew = torch.full((n + 1,) if single else (n + 1, 2), 77.0, dtype=torch.float32, device="cuda")
        done = torch.full((n + 1,), fill, dtype=torch.uint8, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert L.crl_draw_raw_delta(env._h, C.c_void_p(buf.data_ptr()), C.c_void_p(rec.data_ptr()), 0, stream) == 0
        gen = torch.Generator(device="cuda").manual_seed(23)
        dones = 0
        for t in range(steps):
            a = _actions(gen, n, single, "cuda")
            rc = L.crl_step_raw_delta(env._h, C.c_void_p(a.data_ptr()), C.c_void_p(buf.data_ptr()), C.c_void_p(rec.data_ptr()),
                                      C.c_void_p(rew.data_ptr()), C.c_void_p(done.data_ptr()), stream)
            assert rc == 0, L.crl_last_error()
            dones += int(done[:n].sum())
        _assert_whole(env, buf, f"after {steps} steps")
        assert torch.equal(rec[:n], env.obs_descriptors()[6]), "the record does not hold the drawn descriptors"
        assert dones > 0
        assert bool((store[:off] == fill).all()) and bool((store[off + n * per_env:] == fill).all()), "the slack around the buffer was stored to"
        assert int(rec[n]) == sentinel and bool((rew[n:] == 77.0).all()) and int(done[n]) == fill, "an array was written past its n entries"
        # what the call refuses: as crl_draw_raw_delta and crl_step do
        args = [C.c_void_p(a.data_ptr()), C.c_void_p(buf.data_ptr()), C.c_void_p(rec.data_ptr()), C.c_void_p(rew.data_ptr()), C.c_void_p(done.data_ptr())]
        for i in range(3):
            assert L.crl_step_raw_delta(env._h, *[None if j == i else v for j, v in enumerate(args)], stream) == -1
        assert L.crl_step_raw_delta(env._h, args[0], C.c_void_p(buf.data_ptr() + 8), *args[2:], stream) == -1
        assert L.crl_step_raw_delta(env._h, args[0], args[1], C.c_void_p(rec.data_ptr() + 4), *args[3:], stream) == -1
        _assert_whole(env, buf, "after the refused calls")
    finally:
        env.close()
