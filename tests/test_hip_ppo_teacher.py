"""Teacher targets on both learners (include/crl.h "ppo update, teacher targets"; csrc/pong_ppo.hip, pong_ppo_full.hip) and RULE_BASED's
labels (crl_rule_labels) on the device, on the batches, teachers and budgets of tests/ppo_teacher_cases.py (references only).

1. Every gradient tensor and the five PPO statistics plus ce / kl within budget; labelled exact; agree within k / B, k = the batch's
samples with a float64 top-two logit gap below twice the logit budget.  Imitation by logits on every batch, the other two modes on the
big batch and (11, 9); the full-size big batch also at scratch_rows = 320.  2. coef 0 with the policy term = the plain gradient, as
numbers.  3. The same call twice: the same bits.  4. step() behind a teacher gradient is the written Adam; update(teacher=) is the
explicit sequence.  5. Forty imitation steps lower the KL.  6. Every refusal, leaving stats() and the last gradient as they were.
7. A teacher update on a held side stream = the default-stream run.  8. rule_labels against its restatement and against the step."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from competitive_rl_amd import _native as NAT  # noqa: E402
from competitive_rl_amd import rules  # noqa: E402
from competitive_rl_amd.ppo import FullPPO, LightPPO, Teacher, blob_views  # noqa: E402
from competitive_rl_amd.rollout import RolloutStorage  # noqa: E402
from competitive_rl_amd.rules import adam_reference  # noqa: E402
from tests import ppo_cases as P  # noqa: E402
from tests import ppo_full_cases as PF  # noqa: E402
from tests import ppo_teacher_cases as TC  # noqa: E402

NETS = {"light": TC.LIGHT, "full": TC.FULL}
GRAD_CASES = ([("light", n, b, "imitation", None) for n, b in P.CASES + P.BIG_CASES] +
              [("light", n, b, m, None) for n, b in ((11, 9),) + P.BIG_CASES for m in ("mixed", "labels")] +
              [("full", n, b, "imitation", None) for n, b in P.CASES + PF.BIG_CASES] +
              [("full", n, b, m, None) for n, b in ((11, 9),) + PF.BIG_CASES for m in ("mixed", "labels")] +
              [("full", n, b, m, PF.BIG_ROWS) for n, b in PF.BIG_CASES for m in TC.MODES])


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X box")


_storages, _teachers, _runs = {}, {}, {}


def storage(net, n):
    """rollout(n) of the net's cases module recorded into a RolloutStorage, once per process"""
    if (net, n) not in _storages:
        st = RolloutStorage(P.T, n, normalize_advantage=True)
        NETS[net].mod.rollout(n).fill(st)
        _storages[(net, n)] = st
    return _storages[(net, n)]


def dev_teacher(net, n):
    """the rollout's teacher arrays on the device, once per process"""
    if (net, n) not in _teachers:
        td = NETS[net].teacher(n)
        _teachers[(net, n)] = {k: torch.from_numpy(v).cuda() for k, v in td.items()}
    return _teachers[(net, n)]


def teacher_of(net, n, mode, **over):
    m, d = TC.MODES[mode], dev_teacher(net, n)
    kw = dict(temperature=TC.TAU, coef=m["coef"], policy_term=bool(m["policy_term"]))
    if m["kind"] == "logits":
        kw["logits"] = d["logits"].reshape(P.T, n, 3)  # (the (T, N, 3) form)
    else:
        kw["labels"], kw["value_targets"] = d["labels"], d["value_targets"]
    return Teacher(**{**kw, **over})


def learner(net, rows=None, **hyper):
    if net == "light":
        return LightPPO(P.chosen()[1], **{**P.HYPER, **hyper})
    return FullPPO(PF.chosen()[1], scratch_rows=rows, **{**P.HYPER, **hyper})


def _host(net, grads):
    return {k: grads[k].cpu().numpy().copy() for k in NETS[net].keys}


def _idx(bt):
    return torch.from_numpy(bt.idx.astype(np.int64)).cuda()


def run(net, n, b, mode, rows):
    key = (net, n, b, mode, rows)
    if key not in _runs:
        bt = NETS[net].batch(n, b, mode)
        lr = learner(net, rows)
        g = _host(net, lr.grad(storage(net, n), _idx(bt), teacher=teacher_of(net, n, mode)))
        _runs[key] = (g, lr.stats(), lr.teacher_stats())
        lr.close()
    return _runs[key]


def _rel_err(got, want, keys):
    out = {}
    for k in keys:
        top = float(np.abs(want[k]).max())
        out[k] = float(np.abs(np.asarray(got[k], np.float64) - want[k]).max()) / top if top > 0 else float(np.abs(got[k]).max())
    return out


@pytest.mark.parametrize("net,n,b,mode,rows", GRAD_CASES)
def test_gradients_and_statistics_against_float64(net, n, b, mode, rows):
    _need_gpu()
    bt = NETS[net].batch(n, b, mode)
    g, st, ts = run(net, n, b, mode, rows)
    keys = NETS[net].keys
    err = _rel_err(g, bt.r64["grads"], keys)
    print("teacher grad %s N %d B %d %s rows %s: " % (net, n, b, mode, rows) +
          "  ".join("%s err %.3g budget %.3g (%.2f)" % (k, err[k], bt.budget[k], err[k] / bt.budget[k]) for k in keys))
    got = dict(zip(P.STAT_KEYS, st[:5]), ce=ts.ce, kl_teacher=ts.kl)
    budget = dict(bt.stat_budget, **bt.teacher_budget)
    print("teacher stats: " + "  ".join("%s %.6g err %.3g budget %.3g" % (k, got[k], abs(got[k] - bt.r64[k]), budget[k]) for k in got) +
          "  agree %.6g (float64 %.6g, near ties %d)  labelled %.6g" % (ts.agreement, bt.r64["agree"], bt.near_ties, ts.labelled))
    for k in keys:
        assert g[k].shape == bt.r64["grads"][k].shape and err[k] <= bt.budget[k], (k, err[k], bt.budget[k])
    for k in got:
        assert abs(got[k] - bt.r64[k]) <= budget[k], (k, got[k], bt.r64[k], budget[k])
    assert ts.labelled == bt.r64["labelled"]
    assert abs(ts.agreement - bt.r64["agree"]) <= (bt.near_ties + 1e-9) / b
    sq = sum(float((g[k].astype(np.float64) ** 2).sum()) for k in keys)
    assert abs(st.grad_norm - np.sqrt(sq)) <= 1e-12 * np.sqrt(sq)


@pytest.mark.parametrize("net,n,b", [("light", 67, 130), ("full", 11, 9)])
def test_coef_zero_with_the_policy_term_is_the_plain_gradient(net, n, b):
    _need_gpu()
    bt = NETS[net].batch(n, b, "imitation")
    lr, st = learner(net), storage(net, n)
    plain = _host(net, lr.grad(st, _idx(bt)))
    plain_stats = lr.stats()
    with pytest.raises(NAT.CrlError, match="no teacher"):
        lr.teacher_stats()
    got = _host(net, lr.grad(st, _idx(bt), teacher=teacher_of(net, n, "imitation", coef=0.0, policy_term=True)))
    for k in NETS[net].keys:
        assert np.array_equal(got[k], plain[k]), k
    assert lr.stats()[:5] == plain_stats[:5]
    assert lr.teacher_stats().labelled == 1.0
    lr.close()


@pytest.mark.parametrize("net,n,b,mode", [("light", 67, 2500, "mixed"), ("full", 67, 601, "labels")])
def test_the_same_call_gives_the_same_bits(net, n, b, mode):
    _need_gpu()
    bt = NETS[net].batch(n, b, mode)
    first, stats, tstats = run(net, n, b, mode, None)
    lr = learner(net)
    for _ in range(2):
        g = _host(net, lr.grad(storage(net, n), _idx(bt), teacher=teacher_of(net, n, mode)))
        assert all(np.array_equal(g[k].view(np.int32), first[k].view(np.int32)) for k in NETS[net].keys)
        assert lr.stats() == stats and lr.teacher_stats() == tstats
    lr.close()


def test_step_behind_a_teacher_gradient_is_the_written_adam():
    _need_gpu()
    net, n, b = "light", 67, 130
    bt = TC.LIGHT.batch(n, b, "imitation")
    hyper = dict(lr=2.5e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5)
    lr = learner(net, **hyper)
    p = lr.weights()
    m, v = {k: np.zeros_like(p[k]) for k in p}, {k: np.zeros_like(p[k]) for k in p}
    for step in (1, 2):
        g = _host(net, lr.grad(storage(net, n), _idx(bt), teacher=teacher_of(net, n, "imitation")))
        norm = lr.stats().grad_norm
        lr.step()
        for k in p:
            p[k], m[k], v[k] = adam_reference(p[k], m[k], v[k], g[k], norm, step, hyper)
        got = lr.weights()
        assert all(np.array_equal(got[k].view(np.int32), p[k].view(np.int32)) for k in p), step
    lr.close()


@pytest.mark.parametrize("net", ["light", "full"])
def test_update_with_a_teacher_is_the_explicit_grad_and_step_sequence(net):
    _need_gpu()
    n, epochs, batches = 11, 2, 3
    st, t = storage(net, n), teacher_of(net, n, "mixed")
    a, b = learner(net), learner(net)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(123)
    a.update(st, epochs, batches, generator=gen, teacher=t)
    gen.manual_seed(123)
    total = P.T * n
    size = total // batches
    for _ in range(epochs):
        perm = torch.randperm(total, device="cuda", generator=gen)
        for k in range(batches):
            b.grad(st, perm[k * size:(k + 1) * size], teacher=t)
            b.step()
    wa, wb = a.weights(), b.weights()
    assert all(np.array_equal(wa[k].view(np.int32), wb[k].view(np.int32)) for k in wa)
    assert a.stats() == b.stats() and a.teacher_stats() == b.teacher_stats() and a.stats().steps == epochs * batches
    c = learner(net)
    gen.manual_seed(123)
    c.update(st, epochs, batches, generator=gen)  # (without the teacher the weights end elsewhere)
    wc = c.weights()
    assert not all(np.array_equal(wa[k], wc[k]) for k in wa)
    a.close(), b.close(), c.close()


def test_forty_imitation_steps_lower_the_kl():
    """A sanity condition on the imitation term ALONE: vf_coef = ent_coef = 0 and the default lr.  (With ppo_cases.HYPER's vf 0.5 and ent
    0.1 the value loss on the rollout's random returns carries the shared features off and the KL RISES, in float64 autograd with the
    written Adam as on the device: 0.045 -> 0.170 at lr 2.5e-4; with both off the same float64 loop gives 0.045 -> 0.010.)"""
    _need_gpu()
    n = 67
    st, t = storage("light", n), teacher_of("light", n, "imitation")
    idx = torch.arange(P.T * n, dtype=torch.int64, device="cuda")
    lr = learner("light", vf_coef=0.0, ent_coef=0.0, lr=2.5e-4)
    lr.grad(st, idx, teacher=t)
    first = lr.teacher_stats().kl
    for _ in range(40):
        lr.step()
        lr.grad(st, idx, teacher=t)
    last = lr.teacher_stats().kl
    print("imitation: kl %.6g -> %.6g" % (first, last))
    assert 0 <= last < first
    lr.close()


@pytest.mark.parametrize("net", ["light", "full"])
def test_refusals_leave_the_learner_as_it_was(net):
    _need_gpu()
    n, b = 11, 9
    bt = NETS[net].batch(n, b, "imitation")
    lr, st, d = learner(net), storage(net, n), dev_teacher(net, n)
    before = _host(net, lr.grad(st, _idx(bt), teacher=teacher_of(net, n, "imitation")))
    stats, tstats = lr.stats(), lr.teacher_stats()
    idx = _idx(bt)
    # the value object
    for kw in (dict(), dict(logits=d["logits"], labels=d["labels"]), dict(logits=d["logits"].double()), dict(labels=d["labels"].long()),
               dict(logits=d["logits"][:, :2]), dict(logits=d["logits"].reshape(-1)), dict(logits=d["logits"].t()),
               dict(logits=d["logits"], value_targets=d["value_targets"][:-1]), dict(logits=d["logits"], value_targets=d["value_targets"].double()),
               dict(logits=d["logits"], temperature=0.0), dict(logits=d["logits"], temperature=float("inf")), dict(logits=d["logits"], coef=-0.5),
               dict(logits=d["logits"], coef=float("nan")), dict(logits=d["logits"], policy_term=2)):
        with pytest.raises(ValueError):
            Teacher(**kw)
    with pytest.raises(ValueError, match="rows"):
        lr.grad(st, idx, teacher=Teacher(logits=d["logits"][:-1]))
    with pytest.raises(ValueError, match="lives on"):
        lr.grad(st, idx, teacher=Teacher(logits=d["logits"].cpu()))
    with pytest.raises(ValueError):
        lr.grad(st, idx, teacher=dict(logits=d["logits"]))
    # the C ABI
    L, hyper, stream, ip = lr._L, lr._hyper(), lr._stream(), ctypes.c_void_p(idx.data_ptr())
    lp, bp, total = d["logits"].data_ptr(), d["labels"].data_ptr(), P.T * n

    def call(count=b, rollout=st._h, index=ip, **over):
        t = NAT.CrlPpoTeacher(**{**dict(logits_dev=lp, labels_dev=None, value_targets_dev=None, rows=total, temperature=2.0, coef=1.0, policy_term=1), **over})
        return L.crl_ppo_grad_teacher(lr._h, rollout, index, count, ctypes.byref(hyper), ctypes.byref(t), stream)

    assert call(labels_dev=bp) == -1 and b"exactly one" in L.crl_last_error()
    assert call(logits_dev=None) == -1 and b"exactly one" in L.crl_last_error()
    assert call(rows=total - 1) == -1 and b"rows" in L.crl_last_error()
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(temperature=bad) == -1 and b"temperature" in L.crl_last_error()
    for bad in (-1.0, float("inf"), float("nan")):
        assert call(coef=bad) == -1 and b"coef" in L.crl_last_error()
    for bad in (-1, 2):
        assert call(policy_term=bad) == -1 and b"policy_term" in L.crl_last_error()
    assert call(count=0) == -1 and call(index=None) == -1 and call(rollout=None) == -1
    assert call(logits_dev=lp + 2) == -1 and b"aligned" in L.crl_last_error()
    good = NAT.CrlPpoTeacher(logits_dev=lp, labels_dev=None, value_targets_dev=None, rows=total, temperature=2.0, coef=1.0, policy_term=1)
    for field, bad in (("clip", -1.0), ("beta1", 1.0), ("eps", 0.0), ("max_grad_norm", 0.0), ("vf_coef", float("nan"))):
        wrong = lr._hyper()
        setattr(wrong, field, bad)
        assert L.crl_ppo_grad_teacher(lr._h, st._h, ip, b, ctypes.byref(wrong), ctypes.byref(good), stream) == -1, field
        assert b"crl_ppo_grad_teacher" in L.crl_last_error()
    assert L.crl_ppo_grad_teacher(lr._h, st._h, ip, b, None, ctypes.byref(good), stream) == -1 and b"hyper" in L.crl_last_error()
    assert L.crl_ppo_grad_teacher(lr._h, st._h, ip, b, ctypes.byref(hyper), None, stream) == -1 and b"null teacher" in L.crl_last_error()
    fresh = RolloutStorage(P.T, n)
    assert call(rollout=fresh._h) == -1 and b"not finished" in L.crl_last_error()
    fresh.close()
    assert L.crl_ppo_teacher_stats(lr._h, None) == -1
    # ... and the learner is as it was
    p = ctypes.c_void_p()
    NAT.check(L.crl_ppo_get_grad(lr._h, ctypes.byref(p), None))
    after = _host(net, blob_views(lr._dev_blob(p.value)))
    assert all(np.array_equal(after[k].view(np.int32), before[k].view(np.int32)) for k in before)
    assert lr.stats() == stats and lr.teacher_stats() == tstats
    assert call() == 0
    lr.close()


@pytest.mark.parametrize("net", ["light", "full"])
def test_a_teacher_update_on_a_held_side_stream_is_the_default_stream_run(net):
    _need_gpu()
    from tests import stream_cases as S

    n = 11
    st, t = storage(net, n), teacher_of(net, n, "labels")
    idx = torch.arange(P.T * n, dtype=torch.int64, device="cuda")
    gen = torch.Generator(device="cuda")
    out = []
    side = S.pick_streams(1)[0]
    for stream in (None, side):
        lr = learner(net)
        gen.manual_seed(7)
        torch.cuda.synchronize()
        if stream is None:
            lr.update(st, 1, 2, generator=gen, teacher=t)
            g = lr.grad(st, idx, teacher=t)
        else:
            with torch.cuda.stream(stream), S.held(stream):
                lr.update(st, 1, 2, generator=gen, teacher=t)
                g = lr.grad(st, idx, teacher=t)
        torch.cuda.synchronize()
        out.append((lr.weights(), _host(net, g), lr.stats(), lr.teacher_stats()))
        lr.close()
    (wa, ga, sa, ta), (wb, gb, sb, tb) = out
    assert all(np.array_equal(wa[k].view(np.int32), wb[k].view(np.int32)) for k in wa)
    assert all(np.array_equal(ga[k].view(np.int32), gb[k].view(np.int32)) for k in ga)
    assert sa == sb and ta == tb


# ---- 8. rule_labels
def _raw_env(n, seed):
    from competitive_rl_amd.vec_env import HipPongVecEnv

    return HipPongVecEnv(n, seed=seed, mode="raw", output="torch")


def _last_round(state, soon):
    """`state` with every env in the last round of its episode (20 rounds played) and, in the envs `soon`, the ball two frames from
    leaving on the left: x = 4 at 4 px a frame, level, at row 40 with the left bat at row 150"""
    st = state.copy()
    st["num_rounds"] = 20
    for i in soon:
        st["ball_x"][i], st["ball_y"][i], st["speed_x"][i], st["speed_y"][i], st["bat_l_y"][i] = 4, 40, -4.0, 0.0, 150
    return st


@pytest.mark.parametrize("n", [1, 7, 130])
def test_rule_labels_are_the_restated_rule_and_what_the_step_resolves(n):
    """a raw context steps one frame per step (skip = 1), so stepping a seat with its label is stepping it with the cheat code"""
    _need_gpu()
    rs = np.random.RandomState(50 + n)
    env, twin = _raw_env(n, 9), _raw_env(n, 9)
    env.reset(), twin.reset()
    # An episode ends at 21 rounds and a round lasts 19 frames at the least, so 60 frames from a reset end none.  Every env therefore
    # starts in its last round (any point ends the episode), and in env 0 and the last env the ball is two frames from the left edge,
    # 100 rows from the left bat, which moves 4 rows a frame: their episodes end at step 1, the other 58 steps play the restarted ones
    start = _last_round(env.get_state(), (0, n - 1))
    env.set_state(start), twin.set_state(start)
    ends = {id(env): 0, id(twin): 0}
    seen = {0: set(), 1: set()}
    out = torch.empty((n,), dtype=torch.int32, device="cuda")
    for step in range(60):
        state = env.get_state()
        labels = {}
        for seat in (0, 1):
            got = env.rule_labels(seat=seat, out=out if seat else None)
            assert got.dtype == torch.int32 and got.shape == (n,)
            labels[seat] = got.cpu().numpy().copy()
            assert np.array_equal(labels[seat], rules.pong_rule_label_reference(state, seat)), (step, seat)
            seen[seat] |= set(labels[seat].tolist())
        after = env.get_state()
        assert after.tobytes() == state.tobytes()  # nothing in the env changed
        # the learner's seat steps with its label here and with 999 in the twin: the same state, every step, through episode ends
        seat = step % 2
        other = rs.randint(0, 3, n).astype(np.int32)
        a, c = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.int32)
        a[:, seat], a[:, 1 - seat] = labels[seat], other
        c[:, seat], c[:, 1 - seat] = 999, other
        for e, acts in ((env, a), (twin, c)):
            ends[id(e)] += int(e.step_device(torch.from_numpy(acts).cuda(), render=False)[2].sum())
        assert env.get_state().tobytes() == twin.get_state().tobytes(), step
    assert ends[id(env)] == ends[id(twin)] >= min(n, 2), ends  # episodes ended, on both, and the labels went on through the restarts
    if n > 1:
        assert seen[0] == {0, 1, 2} and seen[1] == {0, 1, 2}, seen
    with pytest.raises(ValueError):
        env.rule_labels(seat=2)
    with pytest.raises(ValueError):
        env.rule_labels(out=torch.empty((n + 1,), dtype=torch.int32, device="cuda"))
    assert env._L.crl_rule_labels(env._h, 0, ctypes.c_void_p(out.data_ptr()), 0, env._stream()) == -1
    assert env._L.crl_rule_labels(env._h, 3, ctypes.c_void_p(out.data_ptr()), 1, env._stream()) == -1
    assert env._L.crl_rule_labels(env._h, 0, None, 1, env._stream()) == -1
    assert env._L.crl_rule_labels(env._h, 0, ctypes.c_void_p(out.data_ptr() + 2), 1, env._stream()) == -1 and b"aligned" in env._L.crl_last_error()
    env.close(), twin.close()


def test_rule_labels_through_the_wrappers_and_on_a_wrapped_env():
    """TournamentEnvWrapper and LeagueEnvWrapper hand the env's labels on; on a wrapped (skip = 4) env the label is the first frame's"""
    _need_gpu()
    from competitive_rl_amd.league import LeagueEnvWrapper
    from competitive_rl_amd.tournament import TournamentEnvWrapper
    from tests.test_hip_league import _env

    n = 13
    tw = TournamentEnvWrapper(_env(n, 21), n, ["RULE_BASED", "RANDOM"])
    lg = LeagueEnvWrapper(_env(n, 22), n, ["RULE_BASED", "RANDOM"], seed=5)
    for w in (tw, lg):
        w.reset()
        w.env.set_state(_last_round(w.env.get_state(), (0, n - 1)))  # (two envs end their episode inside the first step's four frames)
        ended = 0
        for _ in range(5):
            ended += int(np.asarray(torch.as_tensor(w.step(np.random.RandomState(1).randint(0, 3, n))[2]).cpu()).sum())
            for seat in (0, 1):
                assert np.array_equal(w.rule_labels(seat=seat).cpu().numpy(), rules.pong_rule_label_reference(w.env.get_state(), seat))
        assert ended >= 2, ended
    tw.close(), lg.close()
