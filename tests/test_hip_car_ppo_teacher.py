"""The CarRacing learner's PPO gradient with teacher targets on the device (include/crl.h "car ppo update, teacher targets"; the teacher
instantiation of csrc/car_ppo.hip) against float64 autograd of the written rule (rules.car_ppo_teacher_loss_reference) within the
CPU-derived budgets of tests/car_ppo_teacher_cases.py, per tensor and per statistic, in every mode; coef = 0 against the plain
gradient; the same bits twice; the plain gradient untouched behind a teacher gradient; ``update(teacher=)`` against the hand-written
loop; the refusals.

Measured on an MI355X (device error / budget): see docs/LAB_NOTES_car_ppo_teacher.md."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from competitive_rl_amd import rules as R  # noqa: E402
from tests import car_ppo_cases as Q  # noqa: E402
from tests import car_ppo_teacher_cases as TC  # noqa: E402
from tests.test_hip_car_drivers import _need_gpu, bits  # noqa: E402
from tests.test_hip_car_ppo import filled  # noqa: E402  (the pool in a CarRolloutStorage, once per process)

F = np.float32
_dev = {}


def tensors(mode):
    """(target (T, R, 2), value targets (T, R)) of the cases' teacher data on the device -- once per process, read-only"""
    gauss = TC.MODES[mode][1]
    if gauss not in _dev:
        d = TC.data()
        _dev[gauss] = torch.from_numpy(d.target(mode).reshape(Q.T, Q.ROWS, 2).copy()).cuda()
        _dev["values"] = torch.from_numpy(d.value_targets.reshape(Q.T, Q.ROWS).copy()).cuda()
    return _dev[gauss], _dev["values"]


def teacher_of(mode, **over):
    import competitive_rl_amd as crl

    loss, gauss, pterm, values = TC.MODES[mode]
    target, vt = tensors(mode)
    kw = dict(log_std=TC.data().weights if gauss else None, loss=loss, value_targets=vt if values else None, coef=TC.COEF, policy_term=bool(pterm))
    kw.update(over)
    return crl.CarTeacher(target, **kw)


def idx_of(bt):
    return torch.from_numpy(bt.idx.astype(np.int64)).cuda()


@pytest.mark.parametrize("mode", list(TC.MODES))
@pytest.mark.parametrize("which", TC.WHICH)
def test_teacher_gradient_and_statistics_within_the_budget_and_the_same_bits_twice(which, mode):
    _need_gpu()
    import competitive_rl_amd as crl

    _, storage = filled()
    _, w, _ = Q.chosen()
    bt = TC.batch(which, mode)
    learner = crl.CarPPO(w, **Q.HYPER)
    idx, teacher = idx_of(bt), teacher_of(mode)
    views = learner.grad(storage, idx, teacher)
    blob = learner.grad_blob().cpu().numpy().copy()
    stats, tstats = learner.stats(), learner.teacher_stats()
    assert all(np.array_equal(bits(views[k].cpu().numpy()), bits(R.car_policy_unpack(blob)[k])) for k in Q.KEYS)
    learner.grad(storage, idx, teacher=teacher)
    assert np.array_equal(bits(blob), bits(learner.grad_blob().cpu().numpy())) and learner.stats() == stats and learner.teacher_stats() == tstats
    assert not blob[2505:].any() and np.isfinite(blob).all() and all(np.isfinite(x) for x in tstats)
    assert stats.live == bt.L and stats.steps == 0
    assert tstats.taught == bt.r64["taught"] == bt.Lt / max(bt.L, 1)  # exact: a ratio of two counts
    if bt.L == 0:
        assert not blob.any() and tuple(stats[:6]) == (0.0,) * 6 and tuple(tstats) == (0.0,) * 4
        learner.close()
        return
    err = Q.rel_err(R.car_policy_unpack(blob), bt.r64["grads"])
    print("car ppo teacher %s b %s L %d Lt %d: error / budget %s" % (mode, which, bt.L, bt.Lt, {k: "%.2f" % (err[k] / bt.budget[k]) for k in Q.KEYS}))
    mine = dict(zip(Q.STAT_KEYS, stats[:5]), **dict(zip(TC.T_STAT_KEYS, tstats[:3])))
    serr = {k: abs(mine[k] - bt.r64[k]) for k in TC.STAT_KEYS}
    print("   statistics error / budget %s" % {k: "%.2f" % (serr[k] / bt.stat_budget[k]) for k in TC.STAT_KEYS})
    for k in Q.KEYS:
        assert err[k] <= bt.budget[k], (which, mode, k, err[k], bt.budget[k], bt.e_ref[k])
    for k in TC.STAT_KEYS:
        assert serr[k] <= bt.stat_budget[k], (which, mode, k, serr[k], bt.stat_budget[k])
    learner.close()


@pytest.mark.parametrize("which", [130, "big_tail", "dead"])
def test_coef_zero_is_the_plain_gradient_and_a_plain_gradient_behind_a_teacher_keeps_its_bits(which):
    _need_gpu()
    import competitive_rl_amd as crl

    _, storage = filled()
    _, w, _ = Q.chosen()
    base = TC.base_of(which)
    idx = idx_of(base)
    learner = crl.CarPPO(w, **Q.HYPER)
    plain = {k: v.cpu().numpy().copy() for k, v in learner.grad(storage, idx).items()}
    plain_stats = learner.stats()
    with pytest.raises(crl._native.CrlError, match="no teacher"):
        learner.teacher_stats()
    for mode in ("ce-point-1", "ce-gauss-1", "mse-point-1"):
        got = learner.grad(storage, idx, teacher=teacher_of(mode, coef=0.0))
        for k in Q.KEYS:
            assert np.array_equal(got[k].cpu().numpy(), plain[k]), (mode, k)
        assert learner.stats() == plain_stats
        assert learner.teacher_stats().taught == TC.batch(which, mode).r64["taught"]
    taught = {k: v.cpu().numpy().copy() for k, v in learner.grad(storage, idx, teacher=teacher_of("ce-gauss-1-values")).items()}
    if base.L:
        assert not np.array_equal(taught["policy_w"], plain["policy_w"]) and not np.array_equal(taught["value_w"], plain["value_w"])
    again = learner.grad(storage, idx)
    assert all(np.array_equal(bits(again[k].cpu().numpy()), bits(plain[k])) for k in Q.KEYS) and learner.stats() == plain_stats
    learner.close()


def test_update_with_a_teacher_is_the_hand_written_loop_bit_for_bit():
    _need_gpu()
    import competitive_rl_amd as crl

    _, storage = filled()
    _, w, _ = Q.chosen()
    epochs, batches, total = 2, 3, Q.T * Q.ROWS
    teacher = teacher_of("ce-gauss-1-values")
    a, b = crl.CarPPO(w, **Q.HYPER), crl.CarPPO(w, **Q.HYPER)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(11)
    a.update(storage, epochs, batches, gen, teacher=teacher)
    gen.manual_seed(11)
    size = total // batches
    for _ in range(epochs):
        perm = torch.randperm(total, device="cuda", generator=gen)
        for k in range(batches):
            b.grad(storage, perm[k * size:(k + 1) * size], teacher)
            b.step()
    assert np.array_equal(bits(a._blob()), bits(b._blob())) and a.stats() == b.stats() and a.teacher_stats() == b.teacher_stats()
    assert a.stats().steps == epochs * batches and not np.array_equal(bits(a._blob()), bits(R.car_policy_pack(w)))
    c = crl.CarPPO(w, **Q.HYPER)
    gen.manual_seed(11)
    c.update(storage, epochs, batches, gen)
    assert not np.array_equal(bits(a._blob()), bits(c._blob()))  # (the teacher changed the run)
    a.close(), b.close(), c.close()


def snapshot(learner):
    return learner._blob().tobytes(), learner.grad_blob().cpu().numpy().tobytes(), tuple(learner.stats()), tuple(learner.teacher_stats())


def test_every_refusal_raises_a_value_error_and_leaves_the_learner_alone():
    _need_gpu()
    import competitive_rl_amd as crl

    _, storage = filled()
    _, w, batches = Q.chosen()
    idx = idx_of(batches[65])
    learner = crl.CarPPO(w, **Q.HYPER)
    good = teacher_of("ce-gauss-1-values")
    learner.grad(storage, idx, good)
    before = snapshot(learner)
    target, vt = tensors("ce-gauss-1")
    total = Q.T * Q.ROWS
    bad = [crl.ppo.Teacher(labels=torch.zeros(total, dtype=torch.int32, device="cuda")), dict(target=target), target,
           crl.CarTeacher(target.reshape(-1, 2)[:-1]), crl.CarTeacher(target.cpu()), crl.CarTeacher(target, value_targets=vt.cpu()),
           crl.CarTeacher(torch.zeros((total + 1, 2), device="cuda"))]
    for t in bad:
        with pytest.raises(ValueError):
            learner.grad(storage, idx, teacher=t)
        with pytest.raises(ValueError):
            learner.update(storage, 1, 2, teacher=t)
    for make in (lambda: crl.CarTeacher(target.double()), lambda: crl.CarTeacher(target[..., :1]), lambda: crl.CarTeacher(target, value_targets=vt[:-1]),
                 lambda: crl.CarTeacher(target, coef=float("nan")), lambda: crl.CarTeacher(target, loss="huber"),
                 lambda: crl.CarTeacher(target, log_std=[0.0, float("inf")])):
        with pytest.raises(ValueError):
            make()
    assert snapshot(learner) == before
    # the C ABI's own refusals, before any GPU call (include/crl.h): the native struct, bent one field at a time
    L = crl._native.load()  # (CRL_EINVAL is -1)
    hyper, stream = learner._hyper(), learner._stream()

    def call(**over):
        nat = good._native(learner.device, total)
        for k, v in over.items():
            setattr(nat, k, v)
        return L.crl_car_ppo_grad_teacher(learner._h, storage._h, C.c_void_p(idx.data_ptr()), idx.numel(), C.byref(hyper), C.byref(nat), stream)

    nan2, inf2 = (C.c_float * 2)(float("nan"), 0.0), (C.c_float * 2)(0.0, float("inf"))
    for over in (dict(target_dev=None), dict(rows=total - 1), dict(rows=total + 1), dict(kind=2), dict(kind=-1), dict(point=2), dict(policy_term=-1),
                 dict(policy_term=2), dict(coef=-0.5), dict(coef=float("nan")), dict(coef=float("inf")), dict(teacher_log_std=nan2),
                 dict(teacher_log_std=inf2), dict(target_dev=target.data_ptr() + 4), dict(value_targets_dev=vt.data_ptr() + 2)):
        assert call(**over) == -1, over
    assert L.crl_car_ppo_grad_teacher(learner._h, storage._h, C.c_void_p(idx.data_ptr()), idx.numel(), C.byref(hyper), None, stream) == -1
    assert call(point=1, teacher_log_std=nan2) == 0  # (a point teacher's log_std is not read)
    learner.grad(storage, idx, good)
    assert snapshot(learner) == before
    learner.close()
