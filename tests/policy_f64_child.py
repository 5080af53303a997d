"""Child process of tests/test_hip_policy_f64.py: the light-policy batches, ties and impulses of tests/policy_f64_cases.py through
crl_policy_act with whatever library variant and kernel switch the parent put into the environment (CRL_LIB_VARIANT=abl,
CRL_POLICY_MFMA=0 / 1: both are read once per process).  Writes what the device gave to the .npz named on the command line; the
parent judges it against float64, so nothing here computes a reference.

    python tests/policy_f64_child.py OUT.npz
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from competitive_rl_amd import spaces  # noqa: E402
from competitive_rl_amd.policy_serving import Policy  # noqa: E402
from tests import policy_f64_cases as C  # noqa: E402

CHILD_SIZES = (7, 13, 2059)  # a ragged group of either kernel (groups of 5 and of 8); more groups than persistent workgroups
TIE_ENVS = 9


def abl_library():
    """libcrl_hip_abl.so, the profiling variant that holds the superseded kernels: the one in the tree (build() makes it), built now if
    there is none.  A failure to build it is a failure of the calling test, not a skip."""
    from competitive_rl_amd.build import PKG, build_abl

    path = os.path.join(PKG, "libcrl_hip_abl.so")
    return path if os.path.exists(path) else build_abl()


def light_policy(weights, n):
    return Policy(spaces.Box(0, 255, (1, 42, 42)), spaces.Discrete(3), n, use_light_model=True, weights=weights)


def full_policy(weights, n):
    return Policy(spaces.Box(0, 255, (1, 42, 42)), spaces.Discrete(3), n, use_light_model=False, weights=weights)


def run_calls(pol, frames, first=C.WARMUP):
    """frames [T, n, 42, 42] pushed one per call -> (logits [T - first, n, 3], actions [T - first, n]) of calls first .. T - 1"""
    logits, actions = [], []
    for t in range(frames.shape[0]):
        a = pol.act_device(torch.from_numpy(frames[t][:, None]).cuda(), want_logits=True)
        if t >= first:
            logits.append(pol.logits().cpu().numpy().copy())
            actions.append(a.cpu().numpy().copy())
    return np.stack(logits), np.stack(actions)


def run_ties(make, base, n):
    """actor_w = 0 and each bias of TIE_BIASES: (logits [4 biases, 4 calls, n, 3], actions [4, 4, n]) on dense frames"""
    frames = C.case("medium", "dense").frames_for(n)[:4]
    logits, actions = [], []
    for bias in C.TIE_BIASES:
        pol = make(C.tie_weights(base, bias), n)
        lg, act = run_calls(pol, frames, first=0)
        pol.close()
        logits.append(lg), actions.append(act)
    return np.stack(logits), np.stack(actions)


def run_impulses(pol):
    """The impulse stacks with the ring head in each of its four positions: planes 0 .. 2 go into the ring (set_stack writes them
    relative to the head in force), plane 3 is pushed as the new frame, and every call moves the head on.  logits [4, 25, 3]."""
    st = torch.from_numpy(C.impulse_stacks()).cuda()
    out = []
    for _ in range(4):
        pol.set_stack(torch.roll(st, shifts=1, dims=1))
        pol.act_device(st[:, 3:4].contiguous(), want_logits=True)
        out.append(pol.logits().cpu().numpy().copy())
        assert torch.equal(pol.get_stack(), st)
    return np.stack(out)


def main(out_path):
    out = {}
    for (ws, kind) in C.LIGHT_CASES:
        c = C.case(ws, kind)
        for n in CHILD_SIZES:
            pol = light_policy(c.weights, n)
            lg, act = run_calls(pol, c.frames_for(n))
            pol.close()
            out["%s__%s__%d__logits" % (ws, kind, n)], out["%s__%s__%d__actions" % (ws, kind, n)] = lg, act
    out["tie__logits"], out["tie__actions"] = run_ties(light_policy, C.shipped("medium"), TIE_ENVS)
    pol = light_policy(C.shipped("medium"), len(C.impulse_stacks()))
    out["impulse__logits"] = run_impulses(pol)
    pol.close()
    np.savez(out_path, **out)
    print("policy f64 child ok")


if __name__ == "__main__":
    main(sys.argv[1])
