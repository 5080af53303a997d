"""The host-side rules of the league, the ledger and the arena that need no GPU and no other module of the package: what a play style
may be (``check_sampling``) and the numpy restatements of the device draws (include/crl.h "league draws", "sampled actions") and of
the rollout storage's stack and GAE rules ("rollout storage").  A leaf: ``league``, ``ledger``, ``arena``, ``policy_serving`` and
``rollout`` import it, it imports none of them.
"""
import numpy as np

from . import _native as N


def check_sampling(temperature, epsilon):
    """What ``crl_sampling_set_agent`` / ``crl_policy_set_sampling`` accept, as float32 values: a finite temperature >= 0 (whose
    reciprocal is a float32) and an epsilon in [0, 1]."""
    with np.errstate(over="ignore", divide="ignore"):
        t, e = np.float32(temperature), np.float32(epsilon)
        if not (np.isfinite(t) and t >= 0) or (t > 0 and not np.isfinite(np.float32(1) / t)):
            raise ValueError(f"temperature must be finite and >= 0 (and 1 / temperature a float32), not {temperature}")
    if not 0 <= e <= 1:
        raise ValueError(f"epsilon must lie in [0, 1], not {epsilon}")
    return float(t), float(e)


def sample_eps_q(epsilon):
    """The explore threshold of "sampled actions": min(floor(epsilon * 2^32), 0xFFFFFFFF), in double from the float32 epsilon."""
    return min(int(np.floor(float(np.float32(epsilon)) * 4294967296.0)), 0xFFFFFFFF)


def _philox4x32_10(gid, counter, domain, seed):
    """The four result words (uint64 arrays holding 32 bits) of counter (gid lo, gid hi, counter, domain) under key (seed lo, seed hi)."""
    gid = np.asarray(gid, np.uint64)
    counter = np.asarray(counter, np.uint64)
    shape = np.broadcast(gid, counter).shape
    mask = np.uint64(0xFFFFFFFF)
    c = [np.broadcast_to(gid & mask, shape).copy(), np.broadcast_to(gid >> np.uint64(32), shape).copy(),
         np.broadcast_to(counter & mask, shape).copy(), np.full(shape, int(domain) & 0xFFFFFFFF, np.uint64)]
    k0, k1 = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def league_sample_reference(seed, gid, n, logits, temperature, epsilon):
    """The rule of include/crl.h "sampled actions" in numpy: one Philox4x32-10 call with counter (gid lo, gid hi, n,
    CRL_LEAGUE_DOMAIN_SAMPLE) under the seed gives x0, x1, x2; if x1 < eps_q the action is (x2 * 3) >> 32 (explored); otherwise the
    first-index argmax for ``temperature`` 0; otherwise the inverse-CDF draw of softmax(logits * inv_t) at r = (x0 >> 8) * 2^-24, with
    inv_t = float32(1 / temperature) as the kernels receive it -- computed HERE in float64, so ``margin`` says how far r lay from the
    nearer boundary: min(|r - e0 / S|, |r - (e0 + e1) / S|), inf for greedy and explored draws.  A kernel's float32 ``exp`` may decide a
    draw of tiny margin the other way.  ``gid``, ``n`` broadcast against ``logits[..., 3]``; ``temperature`` / ``epsilon`` are scalars.
    Returns (action int64, explored bool, margin float64).  Host code for tests and for callers that want to predict a draw; the
    kernels do not use it."""
    t, _ = check_sampling(temperature, epsilon)
    lg = np.asarray(logits, np.float64)
    if lg.shape[-1] != 3:
        raise ValueError("logits[..., 3]")
    shape = np.broadcast(np.asarray(gid), np.asarray(n), lg[..., 0]).shape
    x = _philox4x32_10(np.broadcast_to(np.asarray(gid, np.uint64), shape), np.broadcast_to(np.asarray(n, np.uint64), shape),
                       N.CRL_LEAGUE_DOMAIN_SAMPLE, seed)
    lg = np.broadcast_to(lg, shape + (3,))
    explored = x[1] < np.uint64(sample_eps_q(epsilon))
    action = ((x[2] * np.uint64(3)) >> np.uint64(32)).astype(np.int64)
    margin = np.full(shape, np.inf)
    greedy = np.argmax(lg, axis=-1).astype(np.int64)  # (first index on ties)
    if t == 0:
        return np.where(explored, action, greedy), explored, margin
    z = lg * np.float64(np.float32(1) / np.float32(t))
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    s = e.sum(axis=-1)
    b0, b1 = e[..., 0] / s, (e[..., 0] + e[..., 1]) / s
    r = (x[0] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    sampled = np.where(r < b0, 0, np.where(r < b1, 1, 2)).astype(np.int64)
    margin = np.where(explored, np.inf, np.minimum(np.abs(r - b0), np.abs(r - b1)))
    return np.where(explored, action, sampled), explored, margin


def rollout_logp_reference(logits, actions, temperature):
    """The log-probability rule of include/crl.h "rollout heads" in numpy: z_a = l_a * inv_t, m = max z, d_a = z_a - m in float32 exactly
    as the kernels form them (inv_t = float32 1 / temperature, 1 at temperature 0); e_a = exp(d_a), S = (e0 + e1) + e2 and
    logp = d_action - log(S) HERE in float64.  ``actions`` are the actions written, whichever branch chose them: epsilon is not
    folded into the probability.  ``logits[..., 3]`` float32, ``actions[...]`` integers; returns float64.  Host code for tests and
    for callers that want to check a log-prob; the kernels do not use it."""
    t, _ = check_sampling(temperature, 0.0)
    lg = np.asarray(logits, np.float32)
    if lg.shape[-1] != 3:
        raise ValueError("logits[..., 3]")
    inv_t = np.float32(1) / np.float32(t) if t > 0 else np.float32(1)
    z = (lg * inv_t).astype(np.float32)
    d = (z - z.max(axis=-1, keepdims=True)).astype(np.float32)
    e = np.exp(d.astype(np.float64))
    s = (e[..., 0] + e[..., 1]) + e[..., 2]
    a = np.asarray(actions, np.int64)
    if a.shape != lg.shape[:-1] or a.min(initial=0) < 0 or a.max(initial=0) > 2:
        raise ValueError("one action in {0, 1, 2} per row of logits")
    return np.take_along_axis(d, a[..., None], axis=-1)[..., 0].astype(np.float64) - np.log(s)


def league_draw_reference(seed, gid, counter, domain, m):
    """The league's draw rule in numpy (include/crl.h "league draws"): Philox4x32-10 word 0 of counter (gid lo, gid hi, counter,
    domain) under key (seed lo, seed hi), scaled to [0, m) by a multiply-high.  Arrays broadcast; returns int64.  Host code for
    tests and for callers that want to predict an assignment; the kernels do not use it."""
    c = _philox4x32_10(gid, counter, domain, seed)
    return ((c[0] * np.uint64(m)) >> np.uint64(32)).astype(np.int64)


def weighted_draw_reference(seed, gid, counter, domain, weights):
    """The weighted draw over a table of one weight per agent in numpy (include/crl.h "ledger draws"): r = ``league_draw_reference``
    under ``domain`` scaled to the sum T of the weights, which must lie in [1, 2^32); the smallest agent whose cumulative weight exceeds
    r.  ``weights``: non-negative integers, checked by the caller (``ledger.ledger_draw_reference``, ``car_league_draw_reference``)."""
    w = np.asarray(weights)
    total = int(w.astype(np.uint64).sum())
    if not 0 < total < 2 ** 32:
        raise ValueError(f"the weights must sum to a value in [1, 2^32), not {total}")
    r = league_draw_reference(seed, gid, counter, domain, total)  # (x * T) >> 32
    return np.searchsorted(np.cumsum(w.astype(np.int64)), r, side="right").astype(np.int64)


def rollout_stack_reference(rows, reset, depth_before=3):
    """The stack rule of include/crl.h "rollout storage" in numpy.  ``rows``: uint8 [T + 3, N, 42, 42] -- rows 0..2 the three frames before
    step 0 (oldest first), row t + 3 the frame pushed at step t; ``reset``: [T, N], non-zero where the stack was masked before the push;
    ``depth_before``: depth[-1], a scalar or [N] -- 3 after ``begin`` with a stack or on a fresh storage, ``min(3, depth[T - 1])`` of the
    rollout before after a carrying ``begin``.  depth[t] = 1 where reset[t], else min(4, depth[t - 1] + 1); plane j of sample (t, e) is
    row t + j of env e if 3 - j < depth[t][e], else zeros.  Returns (stacks uint8 [T, N, 4, 42, 42], depth uint8 [T, N]).  Host code for
    tests and for callers that want to check a gathered stack; the kernels do not use it."""
    rows = np.asarray(rows, np.uint8)
    flags = np.asarray(reset) != 0
    steps, n = flags.shape
    if rows.shape[:2] != (steps + 3, n):
        raise ValueError(f"rows must be [T + 3, N, ...] = [{steps + 3}, {n}, ...], not {rows.shape}")
    d = np.broadcast_to(np.asarray(depth_before, np.int64), (n,)).copy()
    if d.min(initial=1) < 1 or d.max(initial=1) > 3:
        raise ValueError("depth_before lies in [1, 3]")
    depth = np.zeros((steps, n), np.uint8)
    stacks = np.zeros((steps, n, 4) + rows.shape[2:], np.uint8)
    for t in range(steps):
        d = np.where(flags[t], 1, np.minimum(4, d + 1))
        depth[t] = d
        for j in range(4):
            live = (3 - j) < d
            stacks[t, live, j] = rows[t + j, live]
    return stacks, depth


def gae_reference(rewards, values, dones, last_values, gamma, lam):
    """The GAE rule of include/crl.h "rollout storage" in numpy, float32 with one rounding per operation as the kernel forms it:
    g = float32(gamma), gl = float32(g * float32(lam)); acc = 0; for t = T-1 .. 0: nd = done[t] ? 0 : 1, vnext = last_values at T-1 else
    values[t+1], delta = (rewards[t] + (g * vnext) * nd) - values[t], acc = delta + (gl * nd) * acc, adv[t] = acc, ret[t] = acc +
    values[t].  ``rewards``, ``values``, ``dones``: [T, N]; ``last_values``: [N].  Returns (adv, ret) float32 [T, N].  Host code for
    tests; the kernels do not use it."""
    r, v = np.asarray(rewards, np.float32), np.asarray(values, np.float32)
    nd_all = np.where(np.asarray(dones) != 0, np.float32(0), np.float32(1)).astype(np.float32)
    if not (r.shape == v.shape == nd_all.shape) or r.ndim != 2:
        raise ValueError("rewards, values and dones are [T, N]")
    vnext = np.broadcast_to(np.asarray(last_values, np.float32), r.shape[1:]).astype(np.float32)
    g = np.float32(gamma)
    gl = np.float32(g * np.float32(lam))
    acc = np.zeros(r.shape[1:], np.float32)
    adv, ret = np.zeros_like(r), np.zeros_like(r)
    for t in range(r.shape[0] - 1, -1, -1):
        nd = nd_all[t]
        delta = ((r[t] + (g * vnext).astype(np.float32) * nd).astype(np.float32) - v[t]).astype(np.float32)
        acc = (delta + (gl * nd).astype(np.float32) * acc).astype(np.float32)
        adv[t], ret[t] = acc, (acc + v[t]).astype(np.float32)
        vnext = v[t]
    return adv, ret


PPO_KEYS = ("conv1_w", "conv1_b", "conv2_w", "conv2_b", "actor_w", "actor_b", "critic_w", "critic_b")
PPO_DEFAULTS = dict(clip=0.2, vf_coef=0.5, ent_coef=0.01, lr=2.5e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5)


def _light_forward(F, torch, w, x):
    z1 = F.conv2d(x, w["conv1_w"], w["conv1_b"], stride=2)
    a1 = torch.where(z1 > 0, z1, torch.zeros_like(z1))
    z2 = F.conv2d(a1, w["conv2_w"], w["conv2_b"], stride=2)
    a2 = torch.where(z2 > 0, z2, torch.zeros_like(z2)).reshape(x.shape[0], 1600)
    return a2, dict(z1=z1, z2=z2)


def _full_forward(F, torch, w, x):
    z1 = F.conv2d(x, w["conv1_w"], w["conv1_b"], stride=2)
    a1 = torch.where(z1 > 0, z1, torch.zeros_like(z1))
    z2 = F.conv2d(a1, w["conv2_w"], w["conv2_b"], stride=2, padding=2)
    a2 = torch.where(z2 > 0, z2, torch.zeros_like(z2)).reshape(x.shape[0], 3872)
    z3 = a2 @ w["conv3_w"].reshape(256, 3872).t() + w["conv3_b"]  # (the 11 x 11 convolution over the whole of a2)
    a3 = torch.where(z3 > 0, z3, torch.zeros_like(z3))
    return a3, dict(z1=z1, z2=z2, z3=z3)


def check_teacher(temperature, coef, policy_term):
    """What ``crl_ppo_grad_teacher`` accepts beside its arrays, as the values it receives: a finite float32 temperature > 0, a finite
    float32 coef >= 0 and a policy_term of 0 or 1 (a bool).  Returns (temperature, coef, policy_term) as floats and an int."""
    with np.errstate(over="ignore"):
        t, k = np.float32(temperature), np.float32(coef)
    if not (np.isfinite(t) and t > 0):
        raise ValueError(f"temperature must be finite and > 0, not {temperature}")
    if not (np.isfinite(k) and k >= 0):
        raise ValueError(f"coef must be finite and >= 0, not {coef}")
    if isinstance(policy_term, (bool, np.bool_)):
        policy_term = int(policy_term)
    if not isinstance(policy_term, (int, np.integer)) or int(policy_term) not in (0, 1):
        raise ValueError(f"policy_term must be 0 or 1, not {policy_term!r}")
    return float(t), float(k), int(policy_term)


def _teacher_targets(torch, teacher, count, dtype):
    """(q [B, 3], q log q with the zero terms as 0 [B, 3], labelled [B] bool, what argmax q is taken over [B, 3]) of a per-sample
    teacher dict"""
    logits, labels = teacher.get("logits"), teacher.get("labels")
    if (logits is None) == (labels is None):
        raise ValueError("a teacher has logits or labels, exactly one of the two")
    if logits is not None:
        tau = float(np.float32(teacher.get("temperature", 1.0)))
        u = torch.tensor(np.asarray(logits, np.float32).reshape(count, 3), dtype=dtype) / tau
        logq = torch.log_softmax(u, dim=1)
        q = logq.exp()
        return q, q * logq, torch.ones(count, dtype=torch.bool), u
    lab = np.asarray(labels, np.int64).reshape(count)
    ok = (lab >= 0) & (lab <= 2)
    q = np.zeros((count, 3))
    q[np.nonzero(ok)[0], lab[ok]] = 1.0
    q = torch.tensor(q, dtype=dtype)
    return q, torch.zeros_like(q), torch.tensor(ok), q


def _ppo_loss(keys, forward, weights, stacks, actions, old_logp, returns, adv, hyper, dtype, teacher=None):
    """The loss of include/crl.h "ppo update" behind the features of ``forward``: shared by the references below.  ``teacher``: the
    per-sample teacher dict of ``ppo_teacher_loss_reference`` ("ppo update, teacher targets"), None = the loss as it stands."""
    import torch
    import torch.nn.functional as F

    dtype = torch.float64 if dtype is None else dtype
    h = dict(PPO_DEFAULTS, **(hyper or {}))
    c, vf, ent = (float(np.float32(h[k])) for k in ("clip", "vf_coef", "ent_coef"))
    w = {k: torch.tensor(np.asarray(weights[k], np.float32), dtype=dtype, requires_grad=True) for k in keys}
    x = torch.tensor(np.asarray(stacks, np.uint8).astype(np.float32), dtype=dtype) / 255
    a = torch.tensor(np.asarray(actions, np.int64))
    if teacher is not None and teacher.get("value_targets") is not None:
        returns = np.asarray(teacher["value_targets"], np.float32).reshape(len(a))
    olp, ret, A = (torch.tensor(np.asarray(t, np.float32), dtype=dtype) for t in (old_logp, returns, adv))
    feat, pre = forward(F, torch, w, x)
    logits = feat @ w["actor_w"].t() + w["actor_b"]
    v = (feat @ w["critic_w"].t() + w["critic_b"]).reshape(-1)
    lp_all = torch.log_softmax(logits, dim=1)
    logp = lp_all.gather(1, a[:, None]).reshape(-1)
    ratio = torch.exp(logp - olp)
    policy = -torch.minimum(ratio * A, torch.clamp(ratio, 1 - c, 1 + c) * A)
    value = 0.5 * (ret - v) ** 2
    entropy = -(lp_all.exp() * lp_all).sum(1)
    n = lambda t: t.detach().numpy()  # noqa: E731
    s = lambda t: float(t.detach())  # noqa: E731
    extra = {}
    if teacher is None:
        loss = (policy + vf * value - ent * entropy).mean()
    else:
        _, coef, policy_term = check_teacher(teacher.get("temperature", 1.0), teacher.get("coef", 1.0), teacher.get("policy_term", 1))
        q, qlogq, labelled, order = _teacher_targets(torch, teacher, len(a), dtype)
        ce = -torch.where(q > 0, q * lp_all, torch.zeros_like(lp_all)).sum(1)  # (terms with q_k = 0 count as 0; no label: no term)
        kl_t = ce + qlogq.sum(1)
        loss = (policy_term * policy + coef * ce + vf * value - ent * entropy).mean()
        agree = (np.argmax(n(logits), axis=1) == np.argmax(n(order), axis=1)) & n(labelled)  # (the lowest index among equals)
        extra = dict(ce=s(ce.mean()), kl_teacher=s(kl_t.mean()), agree=float(agree.mean()), labelled=float(n(labelled).mean()), q=n(q))
    loss.backward()
    r = ratio.detach()
    active = ((A >= 0) & (r < 1 + c)) | ((A < 0) & (r > 1 - c))
    return dict(loss=s(loss), policy=s(policy.mean()), value=s(value.mean()), entropy=s(entropy.mean()),
                kl=s((olp - logp).mean()), clipped=float(((r < 1 - c) | (r > 1 + c)).to(dtype).mean()),
                grads={k: n(w[k].grad) for k in keys}, logits=n(logits), v=n(v), logp=n(logp), ratio=n(r),
                active=n(active), **{k: n(z) for k, z in pre.items()}, **extra)


def ppo_loss_reference(weights, stacks, actions, old_logp, returns, adv, hyper=None, dtype=None):
    """The loss of include/crl.h "ppo update" with torch autograd on the CPU; ``dtype=torch.float64`` (the default) is the yardstick of
    the device's gradient.  ``weights``: the eight tensors of ``PPO_KEYS`` in torch layout; ``stacks``: uint8 [B, 4, 42, 42]; ``actions``
    int [B]; ``old_logp``, ``returns``, ``adv`` float [B] (``adv`` as the gather hands it out); ``hyper``: ``clip``, ``vf_coef``,
    ``ent_coef`` (missing ones from ``PPO_DEFAULTS``).  Returns a dict: ``loss``, the five statistics ``policy``, ``value``,
    ``entropy``, ``kl``, ``clipped`` (means over B), ``grads`` (the eight gradient arrays by key) and, per sample, ``z1`` [B, 16, 20, 20],
    ``z2`` [B, 16, 10, 10], ``logits``, ``v``, ``logp``, ``ratio``, ``active`` (the branch with d policy / d logp = -A r).  Host code for
    tests; the kernels do not use it."""
    return _ppo_loss(PPO_KEYS, _light_forward, weights, stacks, actions, old_logp, returns, adv, hyper, dtype)


PPO_FULL_KEYS = ("conv1_w", "conv1_b", "conv2_w", "conv2_b", "conv3_w", "conv3_b", "actor_w", "actor_b", "critic_w", "critic_b")


def ppo_full_loss_reference(weights, stacks, actions, old_logp, returns, adv, hyper=None, dtype=None):
    """``ppo_loss_reference`` for the full-size ActorCritic (include/crl.h "ppo update, full size"): the same loss behind conv1 (4 x 4,
    stride 2), conv2 (4 x 4, stride 2, padding 2) and conv3 (11 x 11 over the whole of a2, written as the 3872 -> 256 product).
    ``weights``: the ten tensors of ``PPO_FULL_KEYS`` in torch layout.  The same return dict, with ``z2`` [B, 32, 11, 11] and, beside it,
    ``z3`` [B, 256].  Host code for tests; the kernels do not use it."""
    return _ppo_loss(PPO_FULL_KEYS, _full_forward, weights, stacks, actions, old_logp, returns, adv, hyper, dtype)


def ppo_teacher_loss_reference(weights, stacks, actions, old_logp, returns, adv, hyper=None, dtype=None, teacher=None):
    """The loss of include/crl.h "ppo update, teacher targets" with torch autograd on the CPU: ``ppo_loss_reference`` plus
    ``coef * ce`` towards a per-sample target distribution, with the policy term switched by ``policy_term``.  ``teacher``: None (then
    this IS ``ppo_loss_reference``) or a dict of PER-SAMPLE rows, already taken at the samples' flat indices: ``logits`` float32
    [B, 3] at ``temperature``, or ``labels`` int [B] (a value outside 0..2: no teacher term for that sample); optionally
    ``value_targets`` float32 [B] in place of the returns; ``temperature`` (1), ``coef`` (1), ``policy_term`` (1).  The return dict
    gains the means ``ce``, ``kl_teacher``, ``agree``, ``labelled`` and the targets ``q`` [B, 3].  Host code for tests."""
    return _ppo_loss(PPO_KEYS, _light_forward, weights, stacks, actions, old_logp, returns, adv, hyper, dtype, teacher)


def ppo_full_teacher_loss_reference(weights, stacks, actions, old_logp, returns, adv, hyper=None, dtype=None, teacher=None):
    """``ppo_teacher_loss_reference`` for the full-size ActorCritic; without a teacher it is ``ppo_full_loss_reference``."""
    return _ppo_loss(PPO_FULL_KEYS, _full_forward, weights, stacks, actions, old_logp, returns, adv, hyper, dtype, teacher)


def pong_rule_label_reference(state, seat):
    """The labels of ``crl_rule_labels`` in numpy over a ``get_state()`` record (``_native.STATE_DT``): the action in 0..2 that the
    cheat code 999 would resolve to for ``seat`` (0 the left bat, 1 the right) on the FIRST frame of the next step.  ``auto_action``
    (pong/base_pong_env.py:457-471) on the ball's speed towards that side (seat 0: ``-speed_x``), the bat's centre ``bat_y + 7`` and
    the ball's centre ``ball_y + 2`` (as the step's decode forms them): a ball moving away sends the bat towards the arena's centre
    line (y = 114), a ball coming is followed, a ball at rest leaves the bat; + 1.  Returns int32 [N].  Host code for tests."""
    if seat not in (0, 1):
        raise ValueError(f"seat must be 0 (left) or 1 (right), not {seat!r}")
    sx = np.asarray(state["speed_x"], np.float64) * (-1.0 if seat == 0 else 1.0)
    bat = np.asarray(state["bat_l_y" if seat == 0 else "bat_r_y"], np.int64) + 7
    ball = np.asarray(state["ball_y"], np.int64) + 2
    centre = 34 + 80
    away = np.where(bat < centre, 1, np.where(bat > centre, -1, 0))
    coming = np.where(bat < ball, 1, -1)
    return (np.where(sx < 0, away, np.where(sx > 0, coming, 0)) + 1).astype(np.int32)


def adam_reference(params, m, v, grad, grad_norm, step, hyper=None):
    """The optimiser step of include/crl.h "ppo update" in numpy float32, one rounding per operation: ``params``, ``m``, ``v``, ``grad``
    float32 arrays of one shape; ``grad_norm``: the float64 square root of the float64 sum of the gradient's squares; ``step``: t, 1 for the first step;
    ``hyper``: ``lr``, ``betas``, ``eps``, ``max_grad_norm``.  Returns the new (params, m, v).  Host code for tests."""
    h = dict(PPO_DEFAULTS, **(hyper or {}))
    f = np.float32
    b1, b2, lr, eps, max_norm = f(h["betas"][0]), f(h["betas"][1]), f(h["lr"]), f(h["eps"]), f(h["max_grad_norm"])
    bc1, bc2 = 1.0 - float(b1) ** int(step), 1.0 - float(b2) ** int(step)
    omb1, omb2, step_size, bc2s = f(1.0 - float(b1)), f(1.0 - float(b2)), f(float(lr) / bc1), f(np.sqrt(bc2))
    norm = f(np.float64(grad_norm))
    coef = min(f(1.0), f(max_norm / f(norm + f(1e-6))))
    p, m, v, g = (np.asarray(t, f) for t in (params, m, v, grad))
    g = (g * coef).astype(f)
    m = ((b1 * m).astype(f) + (omb1 * g).astype(f)).astype(f)
    v = ((b2 * v).astype(f) + (omb2 * (g * g).astype(f)).astype(f)).astype(f)
    denom = ((np.sqrt(v).astype(f) / bc2s).astype(f) + eps).astype(f)
    return (p - (step_size * (m / denom).astype(f)).astype(f)).astype(f), m, v


# ---- include/crl.h "car drivers": the built-in CarRacing agents
CAR_DRIVER_KINDS = ("RANDOM", "RULE_BASED")
CAR_DRIVER_MAX_LOOKAHEAD = 64
CAR_DRIVER_GAS_GAIN = 0.1    # CRL_CAR_DRIVER_GAS_GAIN
CAR_DRIVER_CURVE_SLOW = 0.5  # CRL_CAR_DRIVER_CURVE_SLOW
# the preset of style slot 1 (CRL_CAR_DRIVER_DEFAULT_*), tuned closed loop on the CPU (docs/LAB_NOTES_car_drivers.md)
CAR_DRIVER_DEFAULT_STYLE = dict(kind="RULE_BASED", target_speed=45.0, lookahead=4, steer_gain=1.5, epsilon=0.0)


def check_car_style(kind="RULE_BASED", target_speed=None, lookahead=None, steer_gain=None, epsilon=None):
    """What ``crl_car_driver_set_style`` accepts, as the values it receives: a kind of ``CAR_DRIVER_KINDS`` (name or index), finite
    float32 ``target_speed`` and ``steer_gain`` >= 0, an integer ``lookahead`` in [0, 64] and an ``epsilon`` in [0, 1].  Missing
    parameters are the default style's.  Returns the complete style as a dict (``kind`` as its name)."""
    d = CAR_DRIVER_DEFAULT_STYLE
    if isinstance(kind, str):
        if kind not in CAR_DRIVER_KINDS:
            raise ValueError(f"kind must be one of {CAR_DRIVER_KINDS}, not {kind!r}")
    elif isinstance(kind, (int, np.integer)) and 0 <= int(kind) < len(CAR_DRIVER_KINDS):
        kind = CAR_DRIVER_KINDS[int(kind)]
    else:
        raise ValueError(f"kind must be one of {CAR_DRIVER_KINDS}, not {kind!r}")
    ts = np.float32(d["target_speed"] if target_speed is None else target_speed)
    sg = np.float32(d["steer_gain"] if steer_gain is None else steer_gain)
    la = d["lookahead"] if lookahead is None else lookahead
    e = np.float32(d["epsilon"] if epsilon is None else epsilon)
    for name, v in (("target_speed", ts), ("steer_gain", sg)):
        if not (np.isfinite(v) and v >= 0):
            raise ValueError(f"{name} must be finite and >= 0, not {v}")
    if isinstance(la, bool) or not isinstance(la, (int, np.integer)) or not 0 <= int(la) <= CAR_DRIVER_MAX_LOOKAHEAD:
        raise ValueError(f"lookahead must be an integer in [0, {CAR_DRIVER_MAX_LOOKAHEAD}], not {la!r}")
    if not 0 <= e <= 1:
        raise ValueError(f"epsilon must lie in [0, 1], not {epsilon}")
    return dict(kind=kind, target_speed=float(ts), lookahead=int(la), steer_gain=float(sg), epsilon=float(e))


def car_tile_boxes(tile_poly):
    """The float32 box (x0, y0, x1, y1) of every tile of float32 polygons [..., 5, 2], as the env keeps it (``tile_aabb``): the
    minimum and maximum of the five float32 vertices."""
    p = np.asarray(tile_poly, np.float32)
    return np.concatenate([p.min(axis=-2), p.max(axis=-2)], axis=-1)


def car_driver_draws(seed, gid, car, call):
    """The Philox call of "car drivers": the words (x0, x1, x2, x3) of counter (gid lo, gid hi, call, CRL_CAR_DRIVER_DOMAIN + car)
    under key (seed lo, seed hi), as uint64 arrays holding 32 bits.  ``gid`` and ``call`` broadcast; ``car`` is 0 or 1."""
    return _philox4x32_10(gid, call, N.CRL_CAR_DRIVER_DOMAIN + int(car), seed)


def car_driver_unit(x):
    """A Philox word as a float32 in [-1, 1): float32(int32(x >> 8) - 2^23) * 2^-23 (every step exact)."""
    return ((np.asarray(x, np.uint64) >> np.uint64(8)).astype(np.int64) - (1 << 23)).astype(np.float32) * np.float32(2.0 ** -23)


def _clamp1(x):
    one = np.float32(1)
    return np.where(x < -one, -one, np.where(x > one, one, x)).astype(np.float32)


def car_driver_reference(hull, wheels, done, boxes, n, style, seed, gid, car, call):
    """The rule of include/crl.h "car drivers" in numpy float32, one rounding per operation, bit for bit what ``car_driver_kernel``
    writes for car ``car`` (0 or 1) of E envs at act call ``call``:
      hull    float32 [E, 4]     the car's hull body: cx, cy, vx, vy
      wheels  float32 [E, 4, 2]  the centres of its wheel bodies 0..3 (0, 1 front; 2, 3 rear)
      done    [E]                its done flag
      boxes   float32 [E, T, 4]  the env's tile boxes (x0, y0, x1, y1), ``car_tile_boxes`` of its track; rows >= n are not read
      n       int [E]            the env's tile count
      style   a dict as ``check_car_style`` returns it (missing parameters are the default style's)
      seed, gid [E], call        the key, the GLOBAL env ids and the act-call counter of the draws
    Returns float32 [E, 2]: (steer, gas > 0 / brake < 0).  Host code for tests and for driving the CPU checker; the kernels do not
    use it."""
    f = np.float32
    s = check_car_style(**style)
    hull, wheels, boxes = np.asarray(hull, f), np.asarray(wheels, f), np.asarray(boxes, f)
    E = hull.shape[0]
    if hull.shape != (E, 4) or wheels.shape != (E, 4, 2) or boxes.ndim != 3 or boxes.shape[0] != E or boxes.shape[2] != 4:
        raise ValueError("hull [E, 4], wheels [E, 4, 2], boxes [E, T, 4]")
    n = np.broadcast_to(np.asarray(n, np.int64), (E,))
    done = np.broadcast_to(np.asarray(done), (E,)) != 0
    if n.max(initial=0) > boxes.shape[1]:
        raise ValueError("n exceeds the rows of boxes")
    gid = np.broadcast_to(np.asarray(gid, np.uint64), (E,))
    x = car_driver_draws(seed, gid, car, np.broadcast_to(np.asarray(call, np.uint64), (E,)))
    rnd = np.stack([car_driver_unit(x[0]), car_driver_unit(x[1])], axis=1)
    explore = np.ones(E, bool) if s["kind"] == "RANDOM" else x[2] < np.uint64(sample_eps_q(s["epsilon"]))
    out = np.zeros((E, 2), f)
    half, one, zero = f(0.5), f(1), f(0)
    with np.errstate(all="ignore"):
        live = ~done & (n > 0)
        nn = np.maximum(n, 1)
        tx = (boxes[..., 0] + boxes[..., 2]) * half
        ty = (boxes[..., 1] + boxes[..., 3]) * half
        cx, cy, vx, vy = hull[:, 0], hull[:, 1], hull[:, 2], hull[:, 3]
        dx, dy = tx - cx[:, None], ty - cy[:, None]
        d2 = dx * dx + dy * dy
        d2 = np.where(d2 == d2, d2, f(np.inf))
        d2 = np.where(np.arange(boxes.shape[1])[None, :] < nn[:, None], d2, f(np.inf))
        near = np.argmin(d2, axis=1)  # (the first index among equals)
        goal = (near + s["lookahead"]) % nn
        rows = np.arange(E)
        ax, ay = tx[rows, goal] - cx, ty[rows, goal] - cy
        hx = (wheels[:, 0, 0] + wheels[:, 1, 0]) * half - (wheels[:, 2, 0] + wheels[:, 3, 0]) * half
        hy = (wheels[:, 0, 1] + wheels[:, 1, 1]) * half - (wheels[:, 2, 1] + wheels[:, 3, 1]) * half
        cr = hx * ay - hy * ax
        dt = hx * ax + hy * ay
        den = np.sqrt(hx * hx + hy * hy) * np.sqrt(ax * ax + ay * ay)
        ok = den > zero
        safe = np.where(ok, den, one)
        sn, cs = np.where(ok, cr / safe, zero), np.where(ok, dt / safe, one)
        e = np.where(cs >= zero, sn, np.where(sn > zero, one, np.where(sn < zero, -one, zero))).astype(f)
        steer = _clamp1(-(f(s["steer_gain"]) * e))
        speed = np.sqrt(vx * vx + vy * vy)
        want = f(s["target_speed"]) * (one - f(CAR_DRIVER_CURVE_SLOW) * np.abs(e))
        gas = _clamp1((want - speed) * f(CAR_DRIVER_GAS_GAIN))
    ruled = np.stack([steer, gas], axis=1).astype(f)
    out[live] = np.where(explore[:, None], rnd, ruled)[live]
    return out


# ---- include/crl.h "car policy": the state observation, the reference's MLP on it and the Gaussian draw
CAR_OBS_FEATURES = N.CRL_CAR_OBS_FEATURES
CAR_OBS_SPEED_SCALE, CAR_OBS_DIST_SCALE = 2.0 ** -6, 2.0 ** -5  # CRL_CAR_OBS_SPEED_SCALE, CRL_CAR_OBS_DIST_SCALE
CAR_OBS_OFFSETS = (0, 2, 4, 8, 16)  # tiles ahead of the nearest one whose centres features 6..15 hold
CAR_POLICY_HIDDEN = N.CRL_CAR_POLICY_HIDDEN
CAR_POLICY_SHAPES = dict(fc1_w=(CAR_POLICY_HIDDEN, CAR_OBS_FEATURES), fc1_b=(CAR_POLICY_HIDDEN,), policy_w=(2, CAR_POLICY_HIDDEN), policy_b=(2,),
                         value_w=(1, CAR_POLICY_HIDDEN), value_b=(1,), log_std=(2,))
CAR_POLICY_KEYS = tuple(CAR_POLICY_SHAPES)
_CAR_POLICY_TORCH_KEYS = {"fc1.weight": "fc1_w", "fc1.bias": "fc1_b", "policy.weight": "policy_w", "policy.bias": "policy_b",
                          "value.weight": "value_w", "value.bias": "value_b"}
CAR_POLICY_TWO_PI = np.float32(2 * np.pi)        # CRL_CAR_POLICY_TWO_PI
CAR_POLICY_LN_2PI = np.float32(np.log(2 * np.pi))  # CRL_CAR_POLICY_LN_2PI


def car_policy_weights(weights):
    """The seven arrays of ``CAR_POLICY_KEYS`` as float32, from a dict under those keys or under the keys of a torch ``MLP(21, 2)``
    state dict (``fc1.weight``, ``policy.bias``, ...; numpy arrays or torch tensors), or from the path of a checkpoint holding one
    (``.npz``, or anything ``torch.load`` reads; a ``{"model": state_dict}`` wrapping is looked through).  ``log_std`` is 0 where it is
    missing.  A missing key, a wrong shape or a value that is not finite raises ``ValueError``."""
    import os

    if isinstance(weights, (str, os.PathLike)):
        path = os.fspath(weights)
        if path.endswith(".npz"):
            with np.load(path) as z:
                weights = {k: z[k] for k in z.files}
        else:
            import torch

            weights = torch.load(path, map_location="cpu")
            if isinstance(weights, dict) and isinstance(weights.get("model"), dict):
                weights = weights["model"]
    if not isinstance(weights, dict):
        raise ValueError(f"car policy weights: a dict or a checkpoint path is needed, not {type(weights).__name__}")
    out = {}
    for k, v in weights.items():
        k = _CAR_POLICY_TORCH_KEYS.get(k, k)
        if k in CAR_POLICY_SHAPES:
            v = v.detach().cpu().numpy() if hasattr(v, "detach") else v
            out[k] = np.ascontiguousarray(v, np.float32)
    out.setdefault("log_std", np.zeros(2, np.float32))
    for k, s in CAR_POLICY_SHAPES.items():
        if k not in out:
            raise ValueError(f"car policy weights: {k} is missing")
        if out[k].shape != s:
            raise ValueError(f"car policy weights: {k} has shape {out[k].shape}, the MLP's is {s}")
        if not np.isfinite(out[k]).all():
            raise ValueError(f"car policy weights: {k} holds values that are not finite")
    return {k: out[k] for k in CAR_POLICY_KEYS}


def car_policy_pack(weights):
    """A slot's blob (include/crl.h "car policy": CRL_CAR_POLICY_BLOB_FLOATS float32) from anything ``car_policy_weights`` takes:
    fc1_w transposed, fc1_b, policy_w, value_w, then policy_b, value_b, log_std, std = float32(exp(float64(log_std))) and a pad."""
    w = car_policy_weights(weights)
    std = np.exp(w["log_std"].astype(np.float64)).astype(np.float32)
    blob = np.concatenate([w["fc1_w"].T.reshape(-1), w["fc1_b"], w["policy_w"].reshape(-1), w["value_w"].reshape(-1), w["policy_b"],
                           w["value_b"], w["log_std"], std, np.zeros(1, np.float32)]).astype(np.float32)
    assert blob.size == N.CRL_CAR_POLICY_BLOB_FLOATS
    return blob


def car_policy_unpack(blob):
    """The seven arrays of a blob in torch layout (copies)."""
    b = np.asarray(blob, np.float32).reshape(-1)
    if b.size != N.CRL_CAR_POLICY_BLOB_FLOATS:
        raise ValueError(f"a car policy blob has {N.CRL_CAR_POLICY_BLOB_FLOATS} floats, not {b.size}")
    H, K = CAR_POLICY_HIDDEN, CAR_OBS_FEATURES
    t = K * H + 4 * H
    return dict(fc1_w=b[:K * H].reshape(K, H).T.copy(), fc1_b=b[K * H:K * H + H].copy(), policy_w=b[K * H + H:K * H + 3 * H].reshape(2, H).copy(),
                policy_b=b[t:t + 2].copy(), value_w=b[K * H + 3 * H:t].reshape(1, H).copy(), value_b=b[t + 2:t + 3].copy(), log_std=b[t + 3:t + 5].copy())


def car_obs_reference(hull, wheels, done, visited_count, touch, boxes, n, other_hull=None, other_done=None):
    """The observation of include/crl.h "car policy" in numpy float32, one rounding per operation, bit for bit what
    ``car_policy_kernel`` writes for one car of E envs:
      hull           float32 [E, 6]     the car's hull body: cx, cy, a, vx, vy, w
      wheels         float32 [E, 4, 3]  its wheel bodies 0..3: cx, cy, a
      done           [E]                its done flag
      visited_count  int [E]            tiles it has visited
      touch          bool [E, 4]        wheel k touches at least one tile
      boxes, n                          as ``car_driver_reference`` takes them
      other_hull, other_done            the other car's hull [E, 6] and done flag [E]; None for players == 1
    Returns float32 [E, 21].  Host code for tests and for driving the CPU checker; the kernels do not use it."""
    f = np.float32
    hull, wheels, boxes = np.asarray(hull, f), np.asarray(wheels, f), np.asarray(boxes, f)
    E = hull.shape[0]
    if hull.shape != (E, 6) or wheels.shape != (E, 4, 3) or boxes.ndim != 3 or boxes.shape[0] != E or boxes.shape[2] != 4:
        raise ValueError("hull [E, 6], wheels [E, 4, 3], boxes [E, T, 4]")
    n = np.broadcast_to(np.asarray(n, np.int64), (E,))
    done = np.broadcast_to(np.asarray(done), (E,)) != 0
    touch = np.asarray(touch).reshape(E, 4) != 0
    visited = np.broadcast_to(np.asarray(visited_count, np.int64), (E,))
    if n.max(initial=0) > boxes.shape[1]:
        raise ValueError("n exceeds the rows of boxes")
    half, one, zero = f(0.5), f(1), f(0)
    speed, dist = f(CAR_OBS_SPEED_SCALE), f(CAR_OBS_DIST_SCALE)
    x = np.zeros((E, CAR_OBS_FEATURES), f)
    with np.errstate(all="ignore"):
        live = ~done & (n > 0)
        nn = np.maximum(n, 1)
        cx, cy, a, vx, vy, w = (hull[:, k] for k in range(6))
        hx = (wheels[:, 0, 0] + wheels[:, 1, 0]) * half - (wheels[:, 2, 0] + wheels[:, 3, 0]) * half
        hy = (wheels[:, 0, 1] + wheels[:, 1, 1]) * half - (wheels[:, 2, 1] + wheels[:, 3, 1]) * half
        length = np.sqrt(hx * hx + hy * hy)
        ok = length > zero
        safe = np.where(ok, length, one)
        fx, fy = np.where(ok, hx / safe, one).astype(f), np.where(ok, hy / safe, zero).astype(f)
        lx, ly = -fy, fx

        def frame(px, py, k, scale):
            x[:, k], x[:, k + 1] = (px * fx + py * fy) * scale, (px * lx + py * ly) * scale

        frame(vx, vy, 0, speed)
        x[:, 2] = w * f(0.25)
        x[:, 3] = (wheels[:, 0, 2] - a) * f(2)
        x[:, 4] = touch.sum(axis=1).astype(f) * f(0.25)
        x[:, 5] = visited.astype(f) / nn.astype(f)
        tx = (boxes[..., 0] + boxes[..., 2]) * half
        ty = (boxes[..., 1] + boxes[..., 3]) * half
        dx, dy = tx - cx[:, None], ty - cy[:, None]
        d2 = dx * dx + dy * dy
        d2 = np.where(d2 == d2, d2, f(np.inf))
        d2 = np.where(np.arange(boxes.shape[1])[None, :] < nn[:, None], d2, f(np.inf))
        near = np.argmin(d2, axis=1)  # (the first index among equals)
        rows = np.arange(E)
        for m, o in enumerate(CAR_OBS_OFFSETS):
            g = (near + o) % nn
            frame(tx[rows, g] - cx, ty[rows, g] - cy, 6 + 2 * m, dist)
        if other_hull is not None:
            oh = np.asarray(other_hull, f)
            if oh.shape != (E, 6):
                raise ValueError("other_hull [E, 6]")
            frame(oh[:, 0] - cx, oh[:, 1] - cy, 16, dist)
            frame(oh[:, 3] - vx, oh[:, 4] - vy, 18, speed)
            x[:, 20] = np.where(np.broadcast_to(np.asarray(other_done), (E,)) != 0, zero, one)
    x[~live] = 0
    return x


def car_mlp_reference(weights, obs):
    """Mean and value of the MLP of include/crl.h "car policy" on observations float32 [E, 21], in numpy float32 with the header's
    summation shape -- bit for bit the kernel's.  Returns (mean float32 [E, 2], value float32 [E])."""
    f = np.float32
    w = car_policy_weights(weights)
    x = np.asarray(obs, f)
    E = x.shape[0]
    if x.shape != (E, CAR_OBS_FEATURES):
        raise ValueError(f"obs [E, {CAR_OBS_FEATURES}]")
    H, second = CAR_POLICY_HIDDEN, CAR_POLICY_HIDDEN - 64
    with np.errstate(all="ignore"):
        a = np.broadcast_to(w["fc1_b"], (E, H)).astype(f)
        for k in range(CAR_OBS_FEATURES):
            a = a + w["fc1_w"][None, :, k] * x[:, k, None]
        h = np.where(a > 0, a, f(0)).astype(f)
        lanes = np.arange(64)
        outs = []
        for r, b in ((w["policy_w"][0], w["policy_b"][0]), (w["policy_w"][1], w["policy_b"][1]), (w["value_w"][0], w["value_b"][0])):
            p = h[:, :64] * r[None, :64]
            p[:, :second] = p[:, :second] + h[:, 64:] * r[None, 64:]
            for m in (32, 16, 8, 4, 2, 1):
                p = p + p[:, lanes ^ m]
            outs.append(p[:, 0] + b)
    return np.stack(outs[:2], axis=1).astype(f), outs[2].astype(f)


CAR_TRACK_DOMAIN = 0x43415253  # "CARS"
CAR_TRACK_ATTEMPTS = 256  # attempts of one reset (car_track.hip: kMaxAttempts)


def car_track_counter(episode, attempt, k):
    """Counter word 2 of call ``k`` (0..12) of attempt ``attempt`` (< 256) of episode ``episode`` in "car track draws":
    (episode << 12 | attempt << 4 | k) mod 2^32 -- episode e and e + 2^20 share their counters."""
    episode, attempt, k = int(episode), int(attempt), int(k)
    if not (episode >= 0 and 0 <= attempt < CAR_TRACK_ATTEMPTS and 0 <= k < 13):
        raise ValueError("episode >= 0, attempt in [0, 256), k in [0, 13)")
    return ((episode << 12) | (attempt << 4) | k) & 0xFFFFFFFF


def car_track_uniform(hi, lo):
    """((hi << 32 | lo) >> 11) * 2^-53 of two 32-bit words: a multiple of 2^-53 in [0, 1), exact in float64."""
    x = (np.asarray(hi, np.uint64) << np.uint64(32)) | np.asarray(lo, np.uint64)
    return (x >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


def car_track_words(seed, gid, episode, attempts):
    """The four result words, each uint64 [A, 13], of the 13 Philox4x32-10 calls of every attempt in the sequence ``attempts`` of
    "car track draws": counter (gid lo, gid hi, car_track_counter(episode, attempt, k), "CARS") under key (seed lo, seed hi)."""
    ctr = np.array([[car_track_counter(episode, a, k) for k in range(13)] for a in attempts], np.uint64)
    return _philox4x32_10(np.full(ctr.shape, int(gid) & (2 ** 64 - 1), np.uint64), ctr, CAR_TRACK_DOMAIN, seed)


def car_track_attempts(seed, gid, episode, attempts):
    """``car_track_draws`` of several attempts at once: (u float64 [A, 24], swap int64 [A])."""
    w = car_track_words(seed, gid, episode, attempts)
    u = np.empty((w[0].shape[0], 24), np.float64)
    u[:, 0::2] = car_track_uniform(w[0][:, :12], w[1][:, :12])
    u[:, 1::2] = car_track_uniform(w[2][:, :12], w[3][:, :12])
    return u, (w[0][:, 12] & np.uint64(1)).astype(np.int64)


def car_track_draws(seed, gid, episode, attempt):
    """The draws of one _create_track attempt of a seeded CarRacing context in numpy (include/crl.h "car track draws"): 13
    Philox4x32-10 calls k = 0..12 with counter (gid lo, gid hi, car_track_counter(episode, attempt, k), "CARS") under key
    (seed lo, seed hi); for k < 12 u[2k] = car_track_uniform(w0, w1) and u[2k + 1] = car_track_uniform(w2, w3); swap = w0 & 1 of
    call 12.  ``gid`` = env_id_base + the env's index, ``episode`` = the env's resets so far.  Returns (u float64 [24], swap int):
    a reset takes the track of its first attempt that closes a lap and THAT attempt's swap.  Host code for tests and for callers
    that want to predict a track; the kernels do not use it."""
    u, swap = car_track_attempts(seed, gid, episode, [attempt])
    return u[0], int(swap[0])


def car_policy_draws(seed, gid, car, call):
    """The Philox call of "car policy": as ``car_driver_draws`` under CRL_CAR_POLICY_DOMAIN + car."""
    return _philox4x32_10(gid, call, N.CRL_CAR_POLICY_DOMAIN + int(car), seed)


def car_policy_uniforms(x):
    """(u1 [E, 2] in (0, 1], u2 [E, 2] in [0, 1)) of the four words of ``car_policy_draws``: float32, every step exact."""
    q = [(np.asarray(w, np.uint64) >> np.uint64(8)).astype(np.int64) for w in x]
    s = np.float32(2.0 ** -24)
    return (np.stack([(q[0] + 1).astype(np.float32) * s, (q[2] + 1).astype(np.float32) * s], axis=-1),
            np.stack([q[1].astype(np.float32) * s, q[3].astype(np.float32) * s], axis=-1))


def car_policy_noise(seed, gid, car, call):
    """z float32 [E, 2] of "car policy": Box-Muller of the uniforms in float32, with the float64 logarithm and the float64 cosine of
    the float32 argument each rounded to float32 (the device takes its library's logf, within 1 ulp, and crl_sincosf): z agrees with
    the device's within the header's bound, not bit for bit."""
    f = np.float32
    u1, u2 = car_policy_uniforms(car_policy_draws(seed, gid, car, call))
    with np.errstate(all="ignore"):
        L = np.log(u1.astype(np.float64)).astype(f)
        r = np.sqrt(f(-2) * L)
        t = CAR_POLICY_TWO_PI * u2
        return (r * np.cos(t.astype(np.float64)).astype(f)).astype(f)


def car_policy_noise_bound(seed, gid, car, call):
    """(Z float64 [E, 2], bound float64 [E, 2]): Box-Muller of the same uniforms in float64 and the header's bound on
    |z - Z| = R * 2^-23 * (2 pi + 2), R = sqrt(-2 ln u1)."""
    u1, u2 = car_policy_uniforms(car_policy_draws(seed, gid, car, call))
    R = np.sqrt(-2.0 * np.log(u1.astype(np.float64)))
    return R * np.cos(2 * np.pi * u2.astype(np.float64)), R * 2.0 ** -23 * (2 * np.pi + 2)


def car_policy_sample(mean, log_std, z):
    """(u float32 [E, 2], log_prob float32 [E]) of a sampling slot given its noise z, in the header's written order."""
    f = np.float32
    mean, z, ls = np.asarray(mean, f), np.asarray(z, f), np.asarray(log_std, f).reshape(2)
    std = np.exp(ls.astype(np.float64)).astype(f)
    with np.errstate(all="ignore"):
        u = mean + std[None, :] * z
        t = [(f(-0.5) * z[:, d]) * z[:, d] - ls[d] for d in range(2)]
        return u.astype(f), ((t[0] + t[1]) - CAR_POLICY_LN_2PI).astype(f)


def car_policy_reference(weights, obs, live, deterministic, seed=0, gid=0, car=0, call=0, z=None):
    """What ``crl_car_policy_act`` writes for one served car of E envs: a dict ``u`` [E, 2], ``value`` [E], ``log_prob`` [E], ``z``
    [E, 2], ``mean`` [E, 2].  ``obs`` as ``car_obs_reference`` returns it, ``live`` [E] = not done and n > 0 (the others get zeros);
    ``z``: the noise to use in place of ``car_policy_noise`` (the device's own, for a bit-for-bit comparison of u and log_prob)."""
    f = np.float32
    w = car_policy_weights(weights)
    mean, value = car_mlp_reference(w, obs)
    E = mean.shape[0]
    live = np.broadcast_to(np.asarray(live, bool), (E,))
    if deterministic:
        u, lp, z = mean.copy(), np.zeros(E, f), np.zeros((E, 2), f)
    else:
        gid = np.broadcast_to(np.asarray(gid, np.uint64), (E,))
        z = car_policy_noise(seed, gid, car, np.broadcast_to(np.asarray(call, np.uint64), (E,))) if z is None else np.asarray(z, f).copy()
        u, lp = car_policy_sample(mean, w["log_std"], z)
    out = dict(u=u, value=value.copy(), log_prob=lp, z=z, mean=mean)
    for k in ("u", "value", "log_prob", "z"):
        out[k][~live] = 0
    return out


# ---- include/crl.h "car ppo update": the loss of the car policy's learner
CAR_PPO_DEFAULTS = dict(clip=0.2, vf_coef=0.5, ent_coef=0.0, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, max_grad_norm=0.5)
CAR_PPO_STAT_KEYS = ("policy", "value", "entropy", "kl", "clipped")


CAR_TEACHER_LOSSES = ("ce", "mse")  # enum crl_car_teacher_kind
CAR_TEACHER_STAT_KEYS = ("term", "kl_teacher", "abs_err", "taught")


def check_car_teacher(log_std=None, loss="ce", coef=1.0, policy_term=True):
    """What ``crl_car_ppo_grad_teacher`` accepts beside its arrays, as the values it receives (include/crl.h "car ppo update, teacher
    targets"): ``log_std`` None (a point teacher) or a pair of finite float32 -- or a car policy weight dict or blob, whose
    ``log_std`` is taken --, ``loss`` one of ``CAR_TEACHER_LOSSES``, a finite float32 ``coef`` >= 0 and a ``policy_term`` of 0 or 1 (a
    bool).  Returns (point, (lsq_0, lsq_1) as floats, kind, coef, policy_term); a ``ValueError`` otherwise."""
    if loss not in CAR_TEACHER_LOSSES:
        raise ValueError(f"loss must be one of {CAR_TEACHER_LOSSES}, not {loss!r}")
    if log_std is None:
        point, lsq = 1, (0.0, 0.0)
    else:
        if isinstance(log_std, dict):
            if "log_std" not in log_std:
                raise ValueError("log_std: the weight dict has no log_std")
            log_std = log_std["log_std"]
        try:
            with np.errstate(over="ignore"):
                arr = np.asarray(log_std, np.float32).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError(f"log_std must be None, a pair of floats, a weight dict or a blob, not {type(log_std).__name__}") from None
        if arr.size == N.CRL_CAR_POLICY_BLOB_FLOATS:
            arr = car_policy_unpack(arr)["log_std"]
        if arr.size != 2 or not np.isfinite(arr).all():
            raise ValueError(f"log_std must hold two finite floats, not {arr.tolist() if arr.size <= 8 else arr.shape}")
        point, lsq = 0, (float(arr[0]), float(arr[1]))
    _, k, policy_term = check_teacher(1.0, coef, policy_term)
    return point, lsq, CAR_TEACHER_LOSSES.index(loss), k, policy_term


def car_ppo_loss_reference(weights, obs, actions, old_logp, returns, adv, live, hyper=None, dtype=None):
    """The loss of include/crl.h "car ppo update" with torch autograd on the CPU; ``dtype=torch.float64`` (the default) is the
    yardstick of the device's gradient.  ``weights``: anything ``car_policy_weights`` takes; ``obs`` float32 [B, 21]; ``actions``
    float32 [B, 2]; ``old_logp``, ``returns``, ``adv`` float [B] (``adv`` as the gather hands it out); ``live`` [B]: a dead sample
    contributes nothing, and the sums are divided by max(L, 1) with L the live count; ``hyper``: ``clip``, ``vf_coef``, ``ent_coef``
    (missing ones from ``CAR_PPO_DEFAULTS``).  Returns a dict: ``loss``, the five statistics ``policy``, ``value``, ``entropy``,
    ``kl``, ``clipped`` (means over the live samples), ``live`` (L), ``grads`` (the seven gradient arrays by key) and, per sample,
    ``a`` [B, 100] (the pre-activations), ``mean`` [B, 2], ``v``, ``logp``, ``ratio``, ``active`` (the branch with
    d policy / d logp = -A r).  Host code for tests; the kernels do not use it."""
    return _car_ppo_loss(weights, obs, actions, old_logp, returns, adv, live, hyper, dtype)


def car_ppo_teacher_loss_reference(weights, obs, actions, old_logp, returns, adv, live, hyper=None, dtype=None, teacher=None):
    """The loss of include/crl.h "car ppo update, teacher targets" with torch autograd on the CPU: ``car_ppo_loss_reference`` plus
    ``coef * term`` towards a per-sample target, with the policy term switched by ``policy_term``.  ``teacher``: None (then this IS
    ``car_ppo_loss_reference``) or a dict of PER-SAMPLE rows, already taken at the samples' flat indices: ``target`` float32 [B, 2] (a
    row with a non-finite float: no teacher term for that sample); optionally ``value_targets`` float32 [B] in place of the returns;
    ``log_std`` (None: a point teacher), ``loss`` ("ce"), ``coef`` (1), ``policy_term`` (1) as ``check_car_teacher`` takes them.  The
    return dict gains ``term``, ``kl_teacher`` and ``abs_err`` (means over the Lt taught samples), ``taught`` (Lt / max(L, 1)) and, per
    sample, ``is_taught``.  Host code for tests; the kernels do not use it."""
    return _car_ppo_loss(weights, obs, actions, old_logp, returns, adv, live, hyper, dtype, teacher)


def _car_ppo_loss(weights, obs, actions, old_logp, returns, adv, live, hyper, dtype, teacher=None):
    import math

    import torch

    dtype = torch.float64 if dtype is None else dtype
    h = dict(CAR_PPO_DEFAULTS, **(hyper or {}))
    c, vf, ent = (float(np.float32(h[k])) for k in ("clip", "vf_coef", "ent_coef"))
    w0 = car_policy_weights(weights)
    w = {k: torch.tensor(w0[k], dtype=dtype, requires_grad=True) for k in CAR_POLICY_KEYS}
    x, u = (torch.tensor(np.asarray(t, np.float32), dtype=dtype) for t in (obs, actions))
    if teacher is not None and teacher.get("value_targets") is not None:
        returns = np.asarray(teacher["value_targets"], np.float32).reshape(len(x))
    olp, ret, A = (torch.tensor(np.asarray(t, np.float32), dtype=dtype) for t in (old_logp, returns, adv))
    lv = torch.tensor(np.asarray(live) != 0)
    a = x @ w["fc1_w"].t() + w["fc1_b"]
    hid = torch.where(a > 0, a, torch.zeros_like(a))
    mean = hid @ w["policy_w"].t() + w["policy_b"]
    v = (hid @ w["value_w"].t() + w["value_b"]).reshape(-1)
    ls = w["log_std"]
    zz = (u - mean) / torch.exp(ls)
    logp = (-0.5 * zz ** 2 - ls).sum(1) - math.log(2 * math.pi)
    ratio = torch.exp(logp - olp)
    policy = -torch.minimum(ratio * A, torch.clamp(ratio, 1 - c, 1 + c) * A)
    value = 0.5 * (ret - v) ** 2
    entropy = (ls[0] + ls[1] + (1 + math.log(2 * math.pi))) * torch.ones_like(v)
    L = max(int(lv.sum()), 1)
    zero = torch.zeros_like(v)
    over = lambda t: torch.where(lv, t, zero).sum() / L  # noqa: E731
    n = lambda t: t.detach().numpy()  # noqa: E731
    s = lambda t: float(t.detach())  # noqa: E731
    extra = {}
    if teacher is None:
        loss = over(policy + vf * value - ent * entropy)
    else:
        point, lsq, kind, coef, policy_term = check_car_teacher(teacher.get("log_std"), teacher.get("loss", "ce"), teacher.get("coef", 1.0),
                                                                teacher.get("policy_term", 1))
        tg = np.asarray(teacher["target"], np.float32).reshape(len(x), 2)
        finite = np.isfinite(tg).all(1)
        taught = lv & torch.tensor(finite)
        t = torch.tensor(np.where(finite[:, None], tg, np.float32(0)), dtype=dtype)  # (an untaught row is never looked at: selected out below)
        sq = torch.tensor([0.0, 0.0] if point else [math.exp(2.0 * lsq[0]), math.exp(2.0 * lsq[1])], dtype=dtype)
        dm = mean - t
        sd = torch.exp(ls)
        var = sd * sd
        if CAR_TEACHER_LOSSES[kind] == "ce":
            per = ls + (sq + dm ** 2) / (2 * var)
            term = (per[:, 0] + per[:, 1]) + math.log(2 * math.pi)
            kl_t = term - ((lsq[0] + lsq[1]) + (1 + math.log(2 * math.pi))) if not point else zero
        else:
            term, kl_t = 0.5 * (dm[:, 0] ** 2 + dm[:, 1] ** 2), zero
        loss = over(policy_term * policy + vf * value - ent * entropy + coef * torch.where(taught, term, zero))
        Lt = max(int(taught.sum()), 1)
        among = lambda q: s(torch.where(taught, q, zero).sum() / Lt)  # noqa: E731
        extra = dict(term=among(term), kl_teacher=among(kl_t), abs_err=among((dm[:, 0].abs() + dm[:, 1].abs()) / 2),
                     taught=int(taught.sum()) / L, is_taught=n(taught))
    loss.backward()
    r = ratio.detach()
    active = ((A >= 0) & (r < 1 + c)) | ((A < 0) & (r > 1 - c))
    return dict(loss=s(loss), policy=s(over(policy)), value=s(over(value)), entropy=s(over(entropy)), kl=s(over(olp - logp)),
                clipped=s(over(((r < 1 - c) | (r > 1 + c)).to(dtype))), live=int(lv.sum()),
                grads={k: (n(w[k].grad) if w[k].grad is not None else np.zeros(CAR_POLICY_SHAPES[k])) for k in CAR_POLICY_KEYS},
                a=n(a), mean=n(mean), v=n(v), logp=n(logp), ratio=n(r), active=n(active), **extra)


# ---- include/crl.h "car league": the draw of car 1's driver and the race books
CAR_LEAGUE_KINDS = ("NETWORK", "STYLE")  # enum crl_car_league_kind
CAR_LEAGUE_COUNTER_NAMES = N.CRL_CAR_LEAGUE_COUNTER_NAMES
_CL_A = N.CRL_LEAGUE_MAX_AGENTS


def _car_league_table(weights):
    """``weights`` as the device's table: uint64 (16,), zero beyond the entries given."""
    w = np.asarray(weights)
    if w.ndim != 1 or len(w) > _CL_A or (w < 0).any() or (w > 0xFFFFFFFF).any():
        raise ValueError(f"at most {_CL_A} weights in [0, 2^32)")
    table = np.zeros(_CL_A, np.uint64)
    table[:len(w)] = w.astype(np.uint64)
    return table


def car_league_draw_reference(seed, gid, counter, weights):
    """The car league's weighted draw in numpy: the rule of include/crl.h "ledger draws" (``ledger.ledger_draw_reference``) with
    CRL_CAR_LEAGUE_DOMAIN as the counter's fourth word.  ``gid`` and ``counter`` broadcast; ``weights`` must sum to a value in
    [1, 2^32).  Returns int64.  Host code for tests and for callers that want to predict a draw; the kernels do not use it."""
    return weighted_draw_reference(seed, gid, counter, N.CRL_CAR_LEAGUE_DOMAIN, _car_league_table(weights))


def car_league_q(x):
    """q of "car league": a float32 return in units of 1/256 as an int64 -- rint(clamp(float64(x) * 256, -2^62, 2^62)) (ties to even)
    for a finite x, 0 otherwise."""
    x = np.asarray(x, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.clip(x.astype(np.float64) * np.float64(256.0), -2.0 ** 62, 2.0 ** 62)
        return np.where(np.isfinite(x), np.rint(np.where(np.isfinite(x), v, 0.0)), 0.0).astype(np.int64)


def car_league_columns(pool, agent):
    """What serving pool entry ``agent[e]`` writes into column 1 of the policy's and of the driver's assignment: (policy column, driver
    column), int32 each.  ``pool``: a sequence of (kind, slot), kind "NETWORK" / "STYLE" (or its enum value).  Entries of ``agent``
    outside the pool give -1 in both (the device leaves such a row as it is)."""
    agent = np.asarray(agent, np.int64)
    net, style = np.full(len(pool) + 1, -1, np.int32), np.full(len(pool) + 1, -1, np.int32)
    for a, (kind, slot) in enumerate(pool):
        kind = CAR_LEAGUE_KINDS[kind] if not isinstance(kind, str) else kind
        if kind not in CAR_LEAGUE_KINDS:
            raise ValueError(f"kind must be one of {CAR_LEAGUE_KINDS}")
        (net if kind == "NETWORK" else style)[a] = int(slot)
    idx = np.where((agent >= 0) & (agent < len(pool)), agent, len(pool))
    return net[idx], style[idx]


def car_league_state(num_envs):
    """A fresh league's state as the replay keeps it: ``agent`` int32 (N,) = -1, ``ret`` float32 (N, 2), ``len`` int32 (N,),
    ``draw_ctr`` uint32 (N,), ``counters`` int64 (7, 16) in the order of ``CAR_LEAGUE_COUNTER_NAMES``."""
    n = int(num_envs)
    return dict(agent=np.full(n, -1, np.int32), ret=np.zeros((n, 2), np.float32), len=np.zeros(n, np.int32), draw_ctr=np.zeros(n, np.uint32),
                counters=np.zeros((N.CRL_CAR_LEAGUE_COUNTERS, _CL_A), np.int64))


def _car_league_redraw(state, where, agents, weights, seed, env_id_base):
    table = _car_league_table(weights)
    table[int(agents):] = 0
    if not 0 < int(table.sum()) < 2 ** 32 or not where.any():
        return  # a table without a draw keeps agent and counter
    e = np.nonzero(where)[0]
    state["agent"][e] = car_league_draw_reference(seed, e.astype(np.uint64) + np.uint64(env_id_base), state["draw_ctr"][e], table).astype(np.int32)
    state["draw_ctr"][e] += np.uint32(1)


def car_league_draw_all_reference(state, agents, weights, seed, env_id_base=0):
    """``crl_car_league_draw_all`` on a copy of ``state``: a fresh draw for every env."""
    state = {k: v.copy() for k, v in state.items()}
    _car_league_redraw(state, np.ones(len(state["agent"]), bool), agents, weights, seed, env_id_base)
    return state


def car_league_reset_agent_reference(state, agent):
    """``crl_car_league_reset_agent`` on a copy of ``state``: the counter column of one pool entry back to zero."""
    state = {k: v.copy() for k, v in state.items()}
    state["counters"][:, int(agent)] = 0
    return state


def car_league_reference(state, rewards, dones, agents, weights, seed, env_id_base=0, redraw=True):
    """The replay of include/crl.h "car league": ``crl_car_league_step`` for every recorded step, in numpy.  ``state``: a dict as
    ``car_league_state`` makes it (not modified); ``rewards`` float32 (T, N, 2) and ``dones`` (T, N) as ``step_device`` returned them;
    ``agents``: the pool's size; ``weights``: the table (one sequence for all steps); ``redraw``: a bool, or one per step.  Returns
    (the state after the last step, int32 (T, N): the agent array after every step).  Host code for tests; the kernels do not use it."""
    rewards, dones = np.asarray(rewards, np.float32), np.asarray(dones) != 0
    steps, n = dones.shape
    if rewards.shape != (steps, n, 2) or len(state["agent"]) != n:
        raise ValueError("rewards (T, N, 2), dones (T, N) and a state of N envs")
    state = {k: v.copy() for k, v in state.items()}
    flags = [bool(redraw)] * steps if isinstance(redraw, (bool, np.bool_, int)) else [bool(x) for x in redraw]
    after = np.zeros((steps, n), np.int32)
    c = state["counters"]
    for t in range(steps):
        ret = (state["ret"] + rewards[t]).astype(np.float32)  # one float32 rounding per add
        length = state["len"] + np.int32(1)
        d = dones[t]
        booked = d & (state["agent"] >= 0) & (state["agent"] < int(agents))
        key = state["agent"][booked].astype(np.int64)
        r0, r1 = ret[booked, 0], ret[booked, 1]
        won, lost = r0 > r1, r0 < r1  # a NaN on either side is neither: a draw
        for plane, value in ((0, np.ones(len(key), np.int64)), (1, won.astype(np.int64)), (2, lost.astype(np.int64)),
                             (3, (~won & ~lost).astype(np.int64)), (4, car_league_q(r0)), (5, car_league_q(r1)),
                             (6, length[booked].astype(np.int64))):
            np.add.at(c[plane], key, value)
        ret[d], length[d] = 0, 0
        state["ret"], state["len"] = ret, length
        if flags[t]:
            _car_league_redraw(state, d, agents, weights, seed, env_id_base)
        after[t] = state["agent"]
    return state, after
