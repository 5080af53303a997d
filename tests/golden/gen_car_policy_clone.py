"""The stored weights of the car policy's sufficiency test (include/crl.h "car policy"; docs/LAB_NOTES_car_policy.md section 5).

    PYTHONDONTWRITEBYTECODE=1 OMP_NUM_THREADS=1 python tests/golden/gen_car_policy_clone.py

Nothing of the reference's code runs here beyond what the CPU checker restates: both cars of the 8 tracks of
``tests/car_scenarios.make_oracle_envs(8, seed0=0)`` are driven for 1000 steps by ``rules.car_driver_reference`` (RULE_BASED, epsilon
0.3), every state is labelled with the epsilon-0 rule's action, and a 21 -> 100 -> 2 MLP is fitted to the labels on
``rules.car_obs_reference``'s observation with CPU torch (Adam, full batch, one thread, seed 0): ``tests/car_policy_cases.py``.
``car_policy_clone.npz``: the seven arrays ``rules.car_policy_weights`` takes (value head and log_std zero).  The GPU tests serve these
weights, and ``tests/test_car_policy_rules.py`` pins the tiles they visit; the same test repeats the fit and checks its quality.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import car_policy_cases as CP  # noqa: E402


def main():
    obs, labels = CP.record_rule_labels()
    weights, loss = CP.fit_clone(obs, labels)
    print("fitted %d samples, mean squared error %.5f" % (len(obs), loss))
    np.savez(os.path.join(HERE, "car_policy_clone.npz"), **weights)


if __name__ == "__main__":
    main()
