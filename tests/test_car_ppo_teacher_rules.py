"""The written rule of include/crl.h "car ppo update, teacher targets" on the CPU: float64 autograd of
rules.car_ppo_teacher_loss_reference against the header's closed forms in numpy float64 on every batch and mode; the plain loss at
coef = 0; the fault models of tests/car_ppo_teacher_cases.py; and the refusals of ``CarTeacher`` / ``rules.check_car_teacher`` that
need no GPU."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from competitive_rl_amd import rules as R  # noqa: E402
from tests import car_ppo_cases as Q  # noqa: E402
from tests import car_ppo_teacher_cases as TC  # noqa: E402

F = np.float32
LN2PI = math.log(2 * math.pi)


def closed_forms(w, idx, mode):
    """The header's rule written out in float64 numpy: the loss, the seven gradients through the closed forms of the heads, and the
    four teacher statistics"""
    po, d = Q.pool(), TC.data()
    loss_kind, gauss, pterm, values = TC.MODES[mode]
    c, vf, ent = (float(F(Q.HYPER[k])) for k in ("clip", "vf_coef", "ent_coef"))
    coef = float(F(TC.COEF))
    w = {k: np.asarray(v, np.float64) for k, v in w.items()}
    g = {k: np.zeros_like(v) for k, v in w.items()}
    ls, sd = w["log_std"], np.exp(w["log_std"])
    var = sd * sd
    lsq = d.log_std.astype(np.float64)
    sq = np.exp(2 * lsq) if gauss else np.zeros(2)
    tgt = d.target(mode)
    live = po.live[idx]
    L = max(int(live.sum()), 1)
    loss, sums, Lt = 0.0, np.zeros(3), 0
    for b, s in enumerate(idx.tolist()):
        if not live[b]:
            continue
        x = po.obs[s].astype(np.float64)
        a = w["fc1_w"] @ x + w["fc1_b"]
        h = np.maximum(a, 0)
        mean, v = w["policy_w"] @ h + w["policy_b"], float(w["value_w"][0] @ h + w["value_b"][0])
        zz = (po.u[s].astype(np.float64) - mean) / sd
        logp = float((-0.5 * zz ** 2 - ls).sum() - LN2PI)
        A, r = float(po.adv[s]), math.exp(logp - float(po.logp[s]))
        policy = -min(r * A, min(max(r, 1 - c), 1 + c) * A)
        gl = -A * r if pterm and ((A >= 0 and r < 1 + c) or (A < 0 and r > 1 - c)) else 0.0
        target_v = float(d.value_targets[s]) if values else float(po.ret[s])
        loss += pterm * policy + vf * 0.5 * (target_v - v) ** 2 - ent * (ls.sum() + 1 + LN2PI)
        dmean, dls, dv = gl * zz / sd, gl * (zz ** 2 - 1) - ent, vf * (v - target_v)
        if np.isfinite(tgt[s]).all():  # taught: selected, never multiplied
            dm = mean - tgt[s].astype(np.float64)
            if loss_kind == "ce":
                term = ((ls[0] + (sq[0] + dm[0] ** 2) / (2 * var[0])) + (ls[1] + (sq[1] + dm[1] ** 2) / (2 * var[1]))) + LN2PI
                t_mean, t_ls = dm / var, 1 - (sq + dm ** 2) / var
            else:
                term, t_mean, t_ls = 0.5 * (dm[0] ** 2 + dm[1] ** 2), dm, np.zeros(2)
            kl = term - ((lsq[0] + lsq[1]) + (1 + LN2PI)) if loss_kind == "ce" and gauss else 0.0
            loss += coef * term
            dmean, dls = dmean + coef * t_mean, dls + coef * t_ls
            sums += (term, kl, (abs(dm[0]) + abs(dm[1])) / 2)
            Lt += 1
        g["policy_w"] += np.outer(dmean, h)
        g["policy_b"] += dmean
        g["value_w"] += dv * h[None]
        g["value_b"] += dv
        g["log_std"] += dls
        da = (w["policy_w"].T @ dmean + w["value_w"][0] * dv) * (a > 0)
        g["fc1_w"] += np.outer(da, x)
        g["fc1_b"] += da
    stats = dict(zip(TC.T_STAT_KEYS, sums / max(Lt, 1)), taught=Lt / L)
    return loss / L, {k: v / L for k, v in g.items()}, stats


@pytest.mark.parametrize("mode", list(TC.MODES))
@pytest.mark.parametrize("which", list(Q.CASES) + ["dead"])
def test_autograd_reference_is_the_headers_closed_forms(which, mode):
    _, w, _ = Q.chosen()
    bt = TC.batch(which, mode)
    loss, g, stats = closed_forms(w, bt.idx, mode)
    ref = bt.r64
    assert abs(loss - ref["loss"]) <= 1e-12 * max(1.0, abs(loss))
    for k in Q.KEYS:
        assert np.abs(g[k] - ref["grads"][k]).max() <= 1e-12 * max(np.abs(g[k]).max(), 1e-300), (k, np.abs(g[k] - ref["grads"][k]).max())
    for k in TC.T_STAT_KEYS:
        assert abs(stats[k] - ref[k]) <= 1e-12 * max(1.0, abs(stats[k])), k
    assert stats["taught"] == ref["taught"]
    if which == "dead":
        assert ref["taught"] == 0 and ref["term"] == 0 and all(not ref["grads"][k].any() for k in Q.KEYS)


def test_the_big_tail_sample_is_the_gradient_and_is_taught():
    _, w, _ = Q.chosen()
    for mode in TC.MODES:
        bt = TC.batch("big_tail", mode)
        assert bt.L == 1 and bt.Lt == 1 and bt.r64["taught"] == 1.0 and len(bt.errs) == 3
        loss, g, stats = closed_forms(w, bt.idx[-1:], mode)
        for k in Q.KEYS:
            assert np.abs(g[k] - bt.r64["grads"][k]).max() <= 1e-12 * np.abs(g[k]).max(), k


@pytest.mark.parametrize("which", [7, 130, "dead"])
def test_coef_zero_with_the_policy_term_and_no_value_targets_is_the_plain_loss_exactly(which):
    _, w, _ = Q.chosen()
    base = TC.base_of(which)
    for mode in ("ce-point-1", "ce-gauss-1", "mse-point-1"):
        got = TC.reference(w, base.idx, mode, coef=0.0)
        for k in Q.KEYS:
            assert np.array_equal(got["grads"][k], base.r64["grads"][k]), (mode, k)
        for k in Q.STAT_KEYS + ("loss", "live"):
            assert got[k] == base.r64[k], (mode, k)
        for dtype in (torch.float32,):
            a, b = TC.reference(w, base.idx, mode, dtype, coef=0.0), Q.pool().reference(w, base.idx, dtype)
            assert all(np.array_equal(a["grads"][k], b["grads"][k]) for k in Q.KEYS)
    none = R.car_ppo_teacher_loss_reference(w, *[x[base.idx] for x in (Q.pool().obs, Q.pool().u, Q.pool().logp, Q.pool().ret, Q.pool().adv, Q.pool().live)],
                                            Q.HYPER)
    assert all(np.array_equal(none["grads"][k], base.r64["grads"][k]) for k in Q.KEYS) and "term" not in none


def test_teacher_data_of_the_cases():
    d, po = TC.data(), Q.pool()
    assert d.untaught.sum() == po.size // TC.UNTAUGHT_EVERY and math.gcd(TC.UNTAUGHT_EVERY, Q.DEAD_EVERY) == 1
    assert (d.untaught & ~po.live).sum() <= po.size // (TC.UNTAUGHT_EVERY * Q.DEAD_EVERY) + 1
    for t in (d.target_gauss, d.target_point):
        bad = ~np.isfinite(t).all(1)
        assert np.array_equal(bad, d.untaught) and np.isnan(t[:, 0]).sum() > 0 and np.isinf(t[:, 1]).sum() > 0
        assert not np.isnan(t[:, 1]).any() and not np.isinf(t[:, 0]).any()
    ok = ~d.untaught
    assert np.abs(d.target_point[ok]).max() <= 1.0  # (a driver's action; these weights' means already lie inside)
    bt = TC.batch(130, "ce-gauss-1")
    assert 0 < bt.Lt < bt.L < bt.b and (bt.live & ~bt.taught).any() and not (bt.taught & ~bt.live).any()
    assert bt.r64["kl_teacher"] > 0 and TC.batch(130, "ce-point-1").r64["kl_teacher"] == 0 and TC.batch(130, "mse-point-0").r64["kl_teacher"] == 0
    # an untaught sample's NaN reaches nothing
    assert all(np.isfinite(bt.r64["grads"][k]).all() for k in Q.KEYS) and all(np.isfinite(bt.r64[k]) for k in TC.STAT_KEYS)


def test_the_gaussian_ce_is_the_cross_entropy_and_its_kl_the_kl():
    """E_q[-log p] by Gauss-Hermite quadrature for q = N(t, sq), p = N(mean, var), one sample; and kl = ce - H(q) >= 0, 0 at p = q"""
    _, w, _ = Q.chosen()
    d, po = TC.data(), Q.pool()
    i = np.array([3])
    r = TC.reference(w, i, "ce-gauss-1")
    mean, ls, t, lsq = r["mean"][0], np.asarray(w["log_std"], np.float64), d.target_gauss[3].astype(np.float64), d.log_std.astype(np.float64)
    xs, ws = np.polynomial.hermite_e.hermegauss(40)
    ce = 0.0
    for k in range(2):
        y = t[k] + math.exp(lsq[k]) * xs
        ce += float((ws / math.sqrt(2 * math.pi) * (0.5 * ((y - mean[k]) / math.exp(ls[k])) ** 2 + ls[k] + 0.5 * LN2PI)).sum())
    assert abs(ce - r["term"]) <= 1e-10 * abs(ce) and r["kl_teacher"] >= 0
    same = dict(w, log_std=d.log_std)
    at = R.car_ppo_teacher_loss_reference(same, po.obs[i], po.u[i], po.logp[i], po.ret[i], po.adv[i], po.live[i], Q.HYPER,
                                          teacher=dict(target=R.car_ppo_loss_reference(same, po.obs[i], po.u[i], po.logp[i], po.ret[i], po.adv[i],
                                                                                       po.live[i])["mean"].astype(F), log_std=d.log_std))
    assert abs(at["kl_teacher"]) <= 1e-6  # (the target is the float32 rounding of the learner's own mean)


@pytest.mark.parametrize("mode", list(TC.MODES))
@pytest.mark.parametrize("which", list(Q.CASES) + ["big_tail"])
def test_every_fault_model_lies_two_budgets_away(which, mode):
    _, w, _ = Q.chosen()
    bt = TC.batch(which, mode)
    shown = {}
    for name in TC.FAULTS:
        m = bt.fault_margin(name, w)
        if m is not None:
            shown[name] = m
            assert m >= 2.0, (which, mode, name, m)
    print(which, mode, {k: round(v, 1) for k, v in shown.items()})
    loss, gauss, pterm, values = TC.MODES[mode]
    if which == 130:
        want = {"target_row_b", "teacher_on_dead", "untaught_as_zero_target", "mean_over_taught", "coef_ignored"}
        want |= ({"no_logstd_term"} if loss == "ce" else set()) | ({"sq_dropped"} if gauss else set())
        want |= ({"policy_term_ignored"} if not pterm else set()) | ({"value_targets_ignored"} if values else set())
        assert set(shown) == want
    if which == "big_tail":
        assert {"target_row_b", "teacher_on_dead", "coef_ignored"} <= set(shown)


def test_check_car_teacher_and_car_teacher_refusals():
    import competitive_rl_amd as crl

    assert R.check_car_teacher() == (1, (0.0, 0.0), 0, 1.0, 1)
    w2 = TC.data().weights
    lsq = tuple(float(x) for x in w2["log_std"])
    assert R.check_car_teacher(w2, "mse", 0.5, False) == (0, lsq, 1, 0.5, 0)
    assert R.check_car_teacher(R.car_policy_pack(w2))[:2] == (0, lsq) and R.check_car_teacher([0.25, -1.0])[1] == (0.25, -1.0)
    for bad in (dict(loss="kl"), dict(coef=-0.1), dict(coef=float("nan")), dict(coef=float("inf")), dict(coef=1e39), dict(policy_term=2),
                dict(policy_term=0.5), dict(log_std=[0.0, float("nan")]), dict(log_std=[0.0, float("inf")]), dict(log_std=[0.0]),
                dict(log_std=[0.0, 1.0, 2.0]), dict(log_std={"fc1_w": 0}), dict(log_std="ce")):
        with pytest.raises(ValueError):
            R.check_car_teacher(**bad)
    t = torch.zeros((12, 2))
    ok = crl.CarTeacher(t.reshape(3, 2, 2, 2), log_std=[0.0, 0.0], loss="mse", value_targets=torch.zeros((3, 4)), coef=0.0, policy_term=False)
    assert (ok.rows, ok.point, ok.kind, ok.coef, ok.policy_term) == (12, 0, 1, 0.0, 0) and crl.CarTeacher(t).point == 1
    for args, kw in (((None,), {}), ((t.numpy(),), {}), ((t.double(),), {}), ((torch.zeros((12, 3)),), {}), ((torch.zeros((24,)),), {}),
                     ((torch.zeros((2, 12, 2))[:, ::2],), {}), ((torch.zeros((1, 2, 3, 2, 2)),), {}), ((t,), dict(value_targets=torch.zeros(11))),
                     ((t,), dict(value_targets=torch.zeros((12, 1, 1, 1)))), ((t,), dict(value_targets=torch.zeros(12, dtype=torch.int32))),
                     ((t,), dict(loss="nll")), ((t,), dict(coef=-1.0)), ((t,), dict(policy_term=3)), ((t,), dict(log_std=[float("nan"), 0.0])),
                     ((torch.zeros(25)[1:].reshape(12, 2),), {})):
        with pytest.raises(ValueError):
            crl.CarTeacher(*args, **kw)
    with pytest.raises(ValueError, match="rows"):
        ok._native(t.device, 13)
    assert ok._native(t.device, 12).rows == 12
