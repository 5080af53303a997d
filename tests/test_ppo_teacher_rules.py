"""CPU checks of the teacher rule (include/crl.h "ppo update, teacher targets") on the references of tests/ppo_teacher_cases.py: the
known answers of the written loss, the restated RULE_BASED label, and every fault model at least 2 x budget away on every batch that
claims it.  No GPU."""
import numpy as np
import pytest
import torch

from competitive_rl_amd import _native as N
from competitive_rl_amd import rules
from tests import ppo_cases as P
from tests import ppo_full_cases as PF
from tests import ppo_teacher_cases as TC

LIGHT_BATCHES = [(n, b, m) for n, b in P.CASES for m in ("imitation", "mixed")] + [(11, 9, "labels"), (67, 130, "labels")]
FULL_BATCHES = [(11, 9, m) for m in TC.MODES] + [(67, 67, "imitation")]


def _args(ro, idx):
    return ro.stacks[idx], ro.actions.reshape(-1)[idx], ro.logp.reshape(-1)[idx], ro.ret[idx], ro.adv[idx], P.HYPER


@pytest.mark.parametrize("net,case", [(TC.LIGHT, (11, 9)), (TC.FULL, (11, 8))])
def test_without_a_teacher_the_new_reference_is_the_old_one_bit_for_bit(net, case):
    bt = net.base(*case)
    old = bt.ro.reference(net.weights(), bt.idx)
    new = net.ref(net.weights(), *_args(bt.ro, bt.idx))
    for k in net.keys:
        assert np.array_equal(old["grads"][k].view(np.int64), new["grads"][k].view(np.int64)), k
    assert all(old[k] == new[k] for k in P.STAT_KEYS) and "ce" not in new


def test_autograd_of_the_cross_entropy_is_p_minus_q():
    rs = np.random.RandomState(3)
    l = torch.tensor(rs.standard_normal((64, 3)) * 3, dtype=torch.float64, requires_grad=True)
    t = rs.standard_normal((64, 3)).astype(np.float32) * 3
    q, _, _, _ = rules._teacher_targets(torch, dict(logits=t, temperature=2.0), 64, torch.float64)
    lp = torch.log_softmax(l, dim=1)
    (-(q * lp).sum()).backward()
    assert float((l.grad - (lp.exp().detach() - q)).abs().max()) <= 1e-12
    # tau = 2 on l is tau = 1 on l / 2, exactly (a division by two is exact)
    q1, _, _, _ = rules._teacher_targets(torch, dict(logits=t / np.float32(2), temperature=1.0), 64, torch.float64)
    assert torch.equal(q, q1)


def test_label_form_is_minus_logp_of_the_label_and_minus_one_contributes_nothing():
    bt = TC.LIGHT.base(11, 9)
    ro, w = bt.ro, TC.LIGHT.weights()
    labels = np.array([0, 1, 2, 2, 1, 0, 1, 2, 0], np.int32)
    r = TC.LIGHT.ref(w, *_args(ro, bt.idx), teacher=dict(labels=labels, coef=1.0, policy_term=0))
    lp = r["logits"] - np.log(np.exp(r["logits"]).sum(1, keepdims=True))
    assert abs(r["ce"] - float(-lp[np.arange(9), labels].mean())) <= 1e-12 and abs(r["kl_teacher"] - r["ce"]) <= 1e-15 and r["labelled"] == 1.0
    # every label -1: the loss is the plain one with the policy term off, whatever coef is
    none = TC.LIGHT.ref(w, *_args(ro, bt.idx), teacher=dict(labels=np.full(9, -1, np.int32), coef=3.0, policy_term=0))
    off = TC.LIGHT.ref(w, *_args(ro, bt.idx), teacher=dict(labels=labels, coef=0.0, policy_term=0))
    assert none["ce"] == 0.0 and none["labelled"] == 0.0 and none["agree"] == 0.0
    for k in TC.LIGHT.keys:
        assert np.array_equal(none["grads"][k], off["grads"][k]), k
    # policy_term 0: the stored advantage and old log-prob play no part in the gradient
    other = TC.LIGHT.ref(w, ro.stacks[bt.idx], ro.actions.reshape(-1)[bt.idx], ro.logp.reshape(-1)[bt.idx] + 0.3, ro.ret[bt.idx], -ro.adv[bt.idx], P.HYPER,
                         teacher=dict(labels=labels, coef=1.0, policy_term=0))
    for k in TC.LIGHT.keys:
        assert np.array_equal(other["grads"][k], r["grads"][k]), k


def test_coef_zero_with_the_policy_term_is_the_plain_gradient():
    bt = TC.LIGHT.batch(11, 9, "imitation")
    r = TC.LIGHT.ref(TC.LIGHT.weights(), *_args(bt.ro, bt.idx), teacher=dict(logits=bt.td["logits"][bt.idx], temperature=TC.TAU, coef=0.0, policy_term=1))
    plain = bt.plain()
    for k in TC.LIGHT.keys:
        assert np.array_equal(r["grads"][k], plain[k]), k


def test_teacher_checks():
    for bad in (dict(temperature=0.0), dict(temperature=float("inf")), dict(temperature=float("nan")), dict(coef=-1.0), dict(coef=float("nan")),
                dict(policy_term=2), dict(policy_term=0.5)):
        with pytest.raises(ValueError):
            rules.check_teacher(**{**dict(temperature=1.0, coef=1.0, policy_term=1), **bad})
    assert rules.check_teacher(2, 0, True) == (2.0, 0.0, 1)
    with pytest.raises(ValueError):
        rules._teacher_targets(torch, dict(), 3, torch.float64)
    with pytest.raises(ValueError):
        rules._teacher_targets(torch, dict(logits=np.zeros((3, 3)), labels=np.zeros(3)), 3, torch.float64)


def test_rule_label_reference_is_auto_action_plus_one():
    st = np.zeros(7, N.STATE_DT)
    st["speed_x"] = [4.0, 4.0, -4.0, -4.0, -4.0, 0.0, 4.0]
    st["ball_y"] = [100, 50, 0, 0, 0, 0, 105]
    st["bat_r_y"] = [50, 120, 100, 107, 120, 9, 100]   # centres 57, 127, 107, 114, 127, 16, 107; the ball's 102, 52, ., ., ., ., 107
    st["bat_l_y"] = [100, 107, 120, 40, 40, 9, 100]
    assert rules.pong_rule_label_reference(st, 1).tolist() == [2, 0, 2, 1, 0, 1, 0]   # coming: follow (a tie moves up); away: centre; rest: stay
    assert rules.pong_rule_label_reference(st, 0).tolist() == [2, 1, 0, 0, 0, 1, 2]   # seat 0 sees -speed_x
    with pytest.raises(ValueError):
        rules.pong_rule_label_reference(st, 2)


def _margins(net, cases):
    out = {}
    for n, b, mode in cases:
        bt = net.batch(n, b, mode)
        for f in TC.FAULTS:
            m = bt.fault_margin(f)
            if m is not None:
                out[(n, b, mode, f)] = m
    return out


def test_every_fault_model_stays_two_budgets_away_light():
    m = _margins(TC.LIGHT, LIGHT_BATCHES)
    print("\n".join("light N %d B %d %s %s: %.3g x budget" % (*k, v) for k, v in sorted(m.items())))
    assert {k[3] for k in m} == set(TC.FAULTS)
    assert all(v >= 2 for v in m.values()), {k: v for k, v in m.items() if v < 2}


def test_every_fault_model_stays_two_budgets_away_full():
    m = _margins(TC.FULL, FULL_BATCHES)
    print("\n".join("full N %d B %d %s %s: %.3g x budget" % (*k, v) for k, v in sorted(m.items())))
    assert {k[3] for k in m} == set(TC.FAULTS)
    assert all(v >= 2 for v in m.values()), {k: v for k, v in m.items() if v < 2}


@pytest.mark.parametrize("net,case", [(TC.LIGHT, (67, 2500)), (TC.FULL, (67, 601))])
def test_big_batches_fault_models(net, case):
    for mode in TC.MODES:
        bt = net.batch(*case, mode)
        assert bt.ref_names == ("forward", "reverse", "seq32")
        for f in TC.FAULTS:
            m = bt.fault_margin(f)
            print("%s N %d B %d %s %s: %s" % (net.name, *case, mode, f, "-" if m is None else "%.3g x budget" % m))
            assert m is None or m >= 2, (mode, f, m)
