"""The bits of both PPO learners on small fixed cases, for a parent-against-branch `diff` (a refactor of the closed forms of
include/crl.h "ppo update" under -ffp-contract=off must not move one): ONE process, one line per result, nothing timed.

    python tools/ab/ppo_bits.py [--only light|full] > bits.txt

It goes through the Python interface alone, so it runs unchanged in a checkout of the parent.  Per case a RolloutStorage is filled from
tests.ppo_cases.rollout(n) / tests.ppo_full_cases.rollout(n), idx comes from a seeded numpy generator (repeats allowed), and the lines are
  grad     sha256 of the gradient tensors grad(storage, idx) returns (views of crl_ppo_get_grad's blob), in key order
  stats    stats() of that gradient as hex floats, and teacher_stats() where there is a teacher
  state    sha256 of the weights, m and v of state_dict() after three grad + step pairs on three further draws of idx
Cases (n, B): light (1, 1), (1, 7) with a partial group, (67, 130), (67, 2500) several groups per workgroup; full size (1, 7), (67, 130)
at the default scratch_rows and at 64 (three chunks), (67, 601) at scratch_rows 320 (two chunks of two slices).
Modes: plain; logits (tau 2, policy_term off); mixed (logits, coef 0.5, policy_term on); labels (every fifth -1) with value targets --
the teacher arrays as tests/ppo_teacher_cases.Net.teacher(n) builds them (their sha256 is printed too: the inputs must agree first).
Needs a GPU; there is no fallback."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from competitive_rl_amd import ppo as PPO  # noqa: E402
from competitive_rl_amd.rollout import RolloutStorage  # noqa: E402
from tests import ppo_cases as P  # noqa: E402
from tests import ppo_full_cases as PF  # noqa: E402
from tests import ppo_teacher_cases as TC  # noqa: E402

LIGHT_CASES = ((1, 1, None), (1, 7, None), (67, 130, None), (67, 2500, None))
FULL_CASES = ((1, 7, None), (67, 130, None), (67, 130, 64), (67, 601, 320))
MODES = ("plain", "logits", "mixed", "labels")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def hexes(values):
    return " ".join(float(x).hex() for x in values)


def sha_dict(d):
    """one sha256 over a dict of tensors or arrays, in key order"""
    h = hashlib.sha256()
    for k in sorted(d):
        v = d[k]
        h.update(np.ascontiguousarray(v.cpu().numpy() if isinstance(v, torch.Tensor) else v).tobytes())
    return h.hexdigest()


def teacher_of(dev, n, mode):
    if mode == "plain":
        return None
    if mode == "labels":
        return PPO.Teacher(labels=dev["labels"], value_targets=dev["value_targets"], policy_term=False)
    kw = dict(coef=1.0, policy_term=False) if mode == "logits" else dict(coef=0.5, policy_term=True)
    return PPO.Teacher(logits=dev["logits"].reshape(P.T, n, 3), temperature=TC.TAU, **kw)


def run(name, net, cases):
    weights = net.mod.perturbed(net.mod.base_weights(), 0.1)
    storages, teachers = {}, {}
    for n, b, rows in cases:
        if n not in storages:
            storages[n] = RolloutStorage(P.T, n, normalize_advantage=True)
            net.mod.rollout(n).fill(storages[n])
            td = net.teacher(n)
            teachers[n] = {k: torch.from_numpy(v).cuda() for k, v in td.items()}
            print("%s n %d teacher %s" % (name, n, " ".join("%s %s" % (k, sha(td[k])) for k in sorted(td))), flush=True)
        rs = np.random.default_rng(1000 * n + b)
        idx = [torch.from_numpy(rs.integers(0, P.T * n, b, dtype=np.int64)).cuda() for _ in range(4)]
        for mode in MODES:
            tag = "%s n %d B %d rows %s %s" % (name, n, b, rows, mode)
            teacher = teacher_of(teachers[n], n, mode)
            kw = dict(teacher=teacher) if teacher is not None else {}
            learner = PPO.LightPPO(weights, **P.HYPER) if name == "light" else PPO.FullPPO(weights, scratch_rows=rows, **P.HYPER)
            print("%s grad %s" % (tag, sha_dict(learner.grad(storages[n], idx[0], **kw))))
            print("%s stats %s" % (tag, hexes(learner.stats())))
            if teacher is not None:
                print("%s teacher_stats %s" % (tag, hexes(learner.teacher_stats())))
            for k in range(1, 4):
                learner.grad(storages[n], idx[k], **kw)
                learner.step()
            sd = learner.state_dict()
            print("%s state steps %d weights %s m %s v %s" % (tag, sd["steps"], sha_dict(sd["weights"]), sha_dict(sd["m"]), sha_dict(sd["v"])), flush=True)
            learner.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=("light", "full"), default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ppo_bits.py runs the learners on the GPU; none is visible")
    if args.only != "full":
        run("light", TC.LIGHT, LIGHT_CASES)
    if args.only != "light":
        run("full", TC.FULL, FULL_CASES)


if __name__ == "__main__":
    main()
