"""The car policy on the CPU (include/crl.h "car policy"): properties of the numpy restatement of the state observation
(``rules.car_obs_reference``, what the GPU tests compare ``car_policy_kernel`` with, bit for bit), the MLP restatement against a float64
forward pass of the reference's MLP within a margin derived from the written summation shape, the noise against a float64 Box-Muller
within the header's bound, the sufficiency of the observation (a net cloned from RULE_BASED drives the checker's tracks), and the
argument refusals of ``crl_car_policy_*`` and of the weight helpers."""
import ctypes
import os

import numpy as np
import pytest

from competitive_rl_amd import rules as R
from tests import car_policy_cases as CP

F = np.float32
U = 2.0 ** -24  # the unit roundoff of float32: a rounded result r of an exact value v has |r - v| <= U |v|
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "car_policy_clone.npz")


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def driven():
    """The checker's 8 tracks after 60 steps of RULE_BASED with epsilon 0.3, car 1 of track 2 marked done: (E, boxes, n)."""
    B, boxes, n = CP.checker_tracks(8)
    style = R.check_car_style(epsilon=0.3)
    for t in range(60):
        acts = np.zeros((8, 2, 2), F)
        for c in range(2):
            hull, wheels = CP._driver_inputs(B.E, c)
            acts[:, c] = R.car_driver_reference(hull, wheels, B.E["done"][:, c], boxes, n, style, 1, np.arange(8), c, t)
        B.step(acts.astype(np.float64))
    E = B.E.copy()
    E["done"][2, 1] = 1
    return E, boxes, n


def test_observation_is_zero_for_a_done_car_and_an_empty_track(driven):
    E, boxes, n = driven
    for c in range(2):
        x = CP.obs_of_batch(E, c, boxes, n)
        assert x.dtype == F and x.shape == (8, 21)
        live = E["done"][:, c] == 0
        assert (bits(x[~live]) == 0).all() and (np.abs(x[live]).sum(axis=1) > 0).all()
    assert (bits(CP.obs_of_batch(E, 0, boxes, 0)) == 0).all()  # n = 0
    # the other car's done flag is feature 20 of the live car beside it
    x0 = CP.obs_of_batch(E, 0, boxes, n)
    assert x0[2, 20] == 0.0 and (np.delete(x0[:, 20], 2) == 1.0).all()


def test_observation_of_one_player_has_no_other_car(driven):
    E, boxes, n = driven
    two, one = CP.obs_of_batch(E, 0, boxes, n), CP.obs_of_batch(E, 0, boxes, n, players=1)
    assert (bits(one[:, 16:]) == 0).all() and np.array_equal(bits(one[:, :16]), bits(two[:, :16]))
    assert (np.abs(two[:, 16:20]).sum(axis=1) > 0).all()


def test_observation_does_not_depend_on_the_shard(driven):
    E, boxes, n = driven
    whole = CP.obs_of_batch(E, 1, boxes, n)
    for order in ([5, 6, 7, 0, 1, 2, 3, 4], [7, 3, 1, 0, 2, 6, 4, 5]):
        parts = [CP.obs_of_batch(E[s], 1, boxes[s], n[s]) for s in (order[:3], order[3:])]
        assert np.array_equal(bits(np.concatenate(parts)), bits(whole[order]))


def test_features_6_and_7_are_the_nearest_tile_in_the_cars_frame(driven):
    E, boxes, n = driven
    x = CP.obs_of_batch(E, 0, boxes, n)
    for i in range(8):
        car = E["car"][i, 0]
        c = np.array([car["hull"]["cx"], car["hull"]["cy"]], np.float64)
        centres = np.stack([(boxes[i, :n[i], 0].astype(np.float64) + boxes[i, :n[i], 2]) / 2, (boxes[i, :n[i], 1].astype(np.float64) + boxes[i, :n[i], 3]) / 2], axis=1)
        d = np.linalg.norm(centres - c, axis=1)
        # the feature's length is the smallest distance (x 2^-5); rotations keep lengths
        assert abs(np.hypot(x[i, 6], x[i, 7]) * 32 - d.min()) < 1e-4 * max(1.0, d.min())
        w = car["wheel"]
        f = np.array([w["cx"][:2].mean() - w["cx"][2:].mean(), w["cy"][:2].mean() - w["cy"][2:].mean()], np.float64)
        f /= np.linalg.norm(f)
        rel = centres[np.argmin(d)] - c
        want = np.array([rel @ f, rel @ np.array([-f[1], f[0]])]) / 32
        assert np.abs(x[i, 6:8] - want).max() < 1e-5
        for m, o in enumerate(R.CAR_OBS_OFFSETS):  # the tiles ahead lie further along the track
            rel = centres[(np.argmin(d) + o) % n[i]] - c
            assert abs(np.hypot(x[i, 6 + 2 * m], x[i, 7 + 2 * m]) * 32 - np.linalg.norm(rel)) < 1e-4 * max(1.0, np.linalg.norm(rel))
    # a car driving along its track looks forward at the tiles ahead
    assert (x[:, 14] > 0).all()


def test_feature_5_rises_with_the_visited_tiles(driven):
    E, boxes, n = driven
    x = CP.obs_of_batch(E, 0, boxes, n)
    assert np.array_equal(x[:, 5], E["tile_visited_count"][:, 0].astype(F) / n.astype(F)) and (x[:, 5] > 0).all()
    more = E.copy()
    more["tile_visited_count"][:, 0] += 7
    y = CP.obs_of_batch(more, 0, boxes, n)
    assert (y[:, 5] > x[:, 5]).all() and np.array_equal(bits(np.delete(y, 5, axis=1)), bits(np.delete(x, 5, axis=1)))
    assert set(np.unique(x[:, 4])) <= {0.0, 0.25, 0.5, 0.75, 1.0} and x[:, 4].max() == 1.0


def test_mlp_reference_equals_a_float64_forward_pass_within_the_summation_shapes_margin(driven):
    """fc1: a hidden unit is its bias and 21 terms, each a rounded product, added one after the other: a term passes through at most
    1 + 21 roundings, so |a_j - A_j| <= gamma(22) (|b_j| + sum_k |w_jk x_k|), gamma(k) = k U / (1 - k U).  Outputs: a term is a rounded
    product and passes through at most 1 (the lane's second unit) + 6 (butterfly) + 1 (bias) additions; the hidden units' own error
    enters through |r_j| (relu does not stretch it): |o - O| <= gamma(9) (|bias| + sum_j |h_j r_j|) + (1 + gamma(9)) sum_j |r_j| e_j."""
    E, boxes, n = driven
    gamma = lambda k: k * U / (1 - k * U)  # noqa: E731
    rs = np.random.RandomState(4)
    obs = np.concatenate([CP.obs_of_batch(E, 0, boxes, n), CP.obs_of_batch(E, 1, boxes, n), rs.uniform(-2, 2, (48, 21)).astype(F)])
    worst = 0.0
    for seed, scale in ((0, 1.0), (1, 4.0), (2, 0.25)):
        w = CP.random_weights(seed, scale)
        mean, value = R.car_mlp_reference(w, obs)
        assert mean.dtype == F and value.dtype == F and mean.shape == (64, 2) and value.shape == (64,)
        m64, v64, h64 = CP.mlp_f64(w, obs)
        W = {k: np.asarray(v, np.float64) for k, v in w.items()}
        x = obs.astype(np.float64)
        e_hid = gamma(22) * (np.abs(W["fc1_b"])[None, :] + np.abs(x) @ np.abs(W["fc1_w"]).T)
        for got, want, r, b in ((mean[:, 0], m64[:, 0], W["policy_w"][0], W["policy_b"][0]), (mean[:, 1], m64[:, 1], W["policy_w"][1], W["policy_b"][1]),
                                (value, v64, W["value_w"][0], W["value_b"][0])):
            margin = gamma(9) * (abs(b) + (h64 + e_hid) @ np.abs(r)) + (1 + gamma(9)) * (e_hid @ np.abs(r))
            err = np.abs(got.astype(np.float64) - want)
            worst = max(worst, float((err / margin).max()))
            assert (err <= margin).all(), (seed, float((err / margin).max()))
        assert (h64 > 0).any(axis=0).sum() > 60 and (h64 == 0).any()  # (both sides of the relu)
    print("car_mlp_reference against float64: largest error / margin %.3f" % worst)
    assert worst > 0.005  # (a float32 evaluation: not the float64 pass itself)


def test_mlp_reference_packs_and_reads_every_weight():
    w = CP.random_weights(9)
    blob = R.car_policy_pack(w)
    assert blob.dtype == F and blob.shape == (2508,) and blob[-1] == 0
    back = R.car_policy_unpack(blob)
    assert all(np.array_equal(bits(back[k]), bits(w[k])) for k in R.CAR_POLICY_KEYS)
    assert np.array_equal(blob[2505:2507], np.exp(w["log_std"].astype(np.float64)).astype(F))
    x = np.random.RandomState(0).uniform(-1, 1, (4, 21)).astype(F)
    base = np.concatenate([a.reshape(4, -1) for a in R.car_mlp_reference(w, x)], axis=1)
    x[:, 0] = 3.0  # unit 99 is switched on by input 0 alone: its weights reach the outputs through the second product of lane 35
    w2 = {k: v.copy() for k, v in w.items()}
    w2["fc1_w"][99], w2["fc1_b"][99] = 0, 0
    w2["fc1_w"][99, 0] = 1.0
    off = np.concatenate([a.reshape(4, -1) for a in R.car_mlp_reference(dict(w2, policy_w=w2["policy_w"] * [[1] * 99 + [0]], value_w=w2["value_w"] * [[1] * 99 + [0]]), x)], axis=1)
    on = np.concatenate([a.reshape(4, -1) for a in R.car_mlp_reference(w2, x)], axis=1)
    assert (on != off).all() and base.shape == (4, 3)
    # a torch MLP state dict is taken as it is, log_std defaults to 0
    import torch

    sd = {"fc1.weight": torch.as_tensor(w["fc1_w"]), "fc1.bias": torch.as_tensor(w["fc1_b"]), "policy.weight": torch.as_tensor(w["policy_w"]),
          "policy.bias": torch.as_tensor(w["policy_b"]), "value.weight": torch.as_tensor(w["value_w"]), "value.bias": torch.as_tensor(w["value_b"])}
    t = R.car_policy_weights(sd)
    assert all(np.array_equal(t[k], w[k]) for k in R.CAR_POLICY_KEYS if k != "log_std") and t["log_std"].tolist() == [0.0, 0.0]


def test_noise_lies_within_the_headers_bound_of_a_float64_box_muller():
    """|z - Z| <= R 2^-23 (2 pi + 2) (include/crl.h "car policy"): 1 ulp of the logarithm and the square root's rounding, the rounded
    2 pi and its product, the cosine's rounding, the last product.  A derived bound; the largest ratio seen is printed."""
    gid = np.arange(1 << 15)
    worst = 0.0
    for seed, car, call in ((0, 0, 0), (77, 1, 5), ((9 << 32) | 11, 0, 4000000000)):
        z = R.car_policy_noise(seed, gid, car, call)
        Z, bound = R.car_policy_noise_bound(seed, gid, car, call)
        assert z.dtype == F and z.shape == (len(gid), 2) and np.isfinite(z).all()
        assert (np.abs(z - Z) <= bound).all()
        worst = max(worst, float((np.abs(z - Z) / np.maximum(bound, 1e-300)).max()))
        assert abs(z.mean()) < 0.02 and abs(z.std() - 1) < 0.02 and abs(np.corrcoef(z[:, 0], z[:, 1])[0, 1]) < 0.02
    print("noise against float64 Box-Muller: largest error / bound %.3f" % worst)
    u1, u2 = R.car_policy_uniforms([np.array([0, 0xFF, 0xFFFFFFFF], np.uint64)] * 4)
    assert u1[:, 0].tolist() == [2.0 ** -24, 2.0 ** -24, 1.0] and u2[:, 1].tolist() == [0.0, 0.0, 1.0 - 2.0 ** -24]
    # the draw is the drivers' generator under its own domain, per car
    w = R.car_policy_draws(5, gid[:4], 1, 3)
    assert [int(a[2]) for a in w] == [int(a[2]) for a in R._philox4x32_10(gid[:4], 3, 0x43525031, 5)]
    assert not np.array_equal(w[0], R.car_driver_draws(5, gid[:4], 1, 3)[0])


def test_sampled_action_and_log_prob_follow_the_written_expressions():
    w = CP.random_weights(3)
    rs = np.random.RandomState(1)
    obs = rs.uniform(-1, 1, (16, 21)).astype(F)
    live = np.arange(16) % 5 != 0
    det = R.car_policy_reference(w, obs, live, True)
    mean, value = R.car_mlp_reference(w, obs)
    assert np.array_equal(bits(det["u"][live]), bits(mean[live])) and (det["log_prob"] == 0).all() and (det["z"] == 0).all()
    assert (bits(det["u"][~live]) == 0).all() and (bits(det["value"][~live]) == 0).all() and np.array_equal(det["value"][live], value[live])
    s = R.car_policy_reference(w, obs, live, False, seed=2, gid=np.arange(16), car=1, call=6)
    z = R.car_policy_noise(2, np.arange(16), 1, 6)
    assert np.array_equal(bits(s["z"][live]), bits(z[live])) and (s["z"][~live] == 0).all()
    std = np.exp(w["log_std"].astype(np.float64))
    lp = (-0.5 * z.astype(np.float64) ** 2 - w["log_std"].astype(np.float64) - 0.5 * np.log(2 * np.pi)).sum(axis=1)
    assert np.abs(s["u"][live] - (mean + std * z)[live]).max() < 1e-6 and np.abs(s["log_prob"][live] - lp[live]).max() < 1e-5
    again = R.car_policy_reference(w, obs, live, False, z=s["z"])
    assert all(np.array_equal(bits(again[k]), bits(s[k])) for k in ("u", "log_prob", "z", "value"))


# ---- sufficiency: a net cloned from RULE_BASED on the observation drives the checker's tracks
# what tests/test_car_driver_rules.py's baselines reach on these tracks in 1000 steps (docs/LAB_NOTES_car_drivers.md): constant full gas
# 12 - 37 tiles, RANDOM 11 - 19
BASELINE_BEST = 37
# REGRESSION PIN of rules.car_obs_reference + rules.car_mlp_reference (not a property of the env): tiles visited per track and car after
# 1000 steps under the weights of tests/golden/car_policy_clone.npz -- the fit below as it came out when the pin was taken.  The
# pin drives the stored weights, not the fresh fit: a fit's last bits may depend on the host's BLAS, the numpy rule's do not.
PINNED_VISITED = [[261, 270], [273, 267], [270, 274], [274, 268], [257, 268], [271, 267], [266, 273], [274, 270]]


def test_a_net_cloned_from_rule_based_drives_every_track():
    x, y = CP.record_rule_labels()
    assert x.shape == (16000, 21) and y.shape == (16000, 2) and (np.abs(y).max(axis=0) == 1).all()
    w, loss = CP.fit_clone(x, y)
    visited, n, left = CP.drive_with_mlp(w)
    share = visited / n[:, None]
    print("fit: mean squared error %.5f on %d samples" % (loss, len(x)))
    print("cloned cars visited", visited.tolist(), "of", n.tolist())
    print("share of the track reached: min %.3f median %.3f (RULE_BASED: 0.725 / 0.808)" % (share.min(), np.median(share)))
    assert not left.any(), "a cloned car left the playfield"
    assert (visited > BASELINE_BEST).all(), visited.tolist()


def test_stored_clone_weights_keep_their_visited_counts():
    with np.load(GOLDEN) as z:
        w = {k: z[k] for k in z.files}
    visited, n, left = CP.drive_with_mlp(w)
    assert not left.any() and (visited > BASELINE_BEST).all()
    assert visited.tolist() == PINNED_VISITED


# ---- argument checks that need no GPU
def test_weight_helpers_refuse_bad_weights(tmp_path):
    w = CP.random_weights(0)
    for bad, text in ((dict(w, fc1_w=w["fc1_w"][:, :20]), "shape"), ({k: v for k, v in w.items() if k != "value_b"}, "missing"),
                      (dict(w, policy_b=np.array([0.0, np.nan], F)), "finite"), (dict(w, log_std=np.array([np.inf, 0], F)), "finite"), ([1, 2], "dict")):
        with pytest.raises(ValueError, match=text):
            R.car_policy_pack(bad)
    with pytest.raises(ValueError, match="2508"):
        R.car_policy_unpack(np.zeros(2507, F))
    with pytest.raises(ValueError, match="obs"):
        R.car_mlp_reference(w, np.zeros((3, 20), F))
    path = tmp_path / "net.npz"
    np.savez(path, **w)
    assert all(np.array_equal(R.car_policy_weights(str(path))[k], w[k]) for k in R.CAR_POLICY_KEYS)
    import torch

    torch.save({"model": {k: torch.as_tensor(v) for k, v in w.items()}}, tmp_path / "net.pt")
    assert all(np.array_equal(R.car_policy_weights(tmp_path / "net.pt")[k], w[k]) for k in R.CAR_POLICY_KEYS)
    from competitive_rl_amd.car_policy import is_car_policy_weights

    assert is_car_policy_weights(w) and is_car_policy_weights(str(path)) and is_car_policy_weights(path)
    assert not is_car_policy_weights("RULE_BASED") and not is_car_policy_weights(lambda obs: obs)


def test_car_policy_needs_a_car_env():
    import competitive_rl_amd as crl

    with pytest.raises(TypeError, match="HipCarVecEnv"):
        crl.CarPolicy(object())
    assert callable(crl.car_obs_reference) and callable(crl.car_mlp_reference) and callable(crl.car_policy_reference)


def test_abi_refuses_bad_arguments_without_gpu():
    from competitive_rl_amd import _native as N

    L = N.load()
    h = ctypes.c_void_p()
    err = lambda: L.crl_last_error()  # noqa: E731
    blob = (ctypes.c_float * N.CRL_CAR_POLICY_BLOB_FLOATS)()
    assert L.crl_car_policy_create(None, 0, ctypes.byref(h)) == -1 and b"null" in err()
    assert L.crl_car_policy_create(None, 0, None) == -1
    for slot in (-1, 8):
        assert L.crl_car_policy_set_weights(None, slot, blob, 0, None) == -1 and b"slot" in err()
        assert L.crl_car_policy_get_weights(None, slot, None, None, None) == -1 and b"slot" in err()
        assert L.crl_car_policy_set_sampling(None, slot, 1) == -1 and b"slot" in err()
    for flag in (-1, 2):
        assert L.crl_car_policy_set_weights(None, 0, blob, flag, None) == -1 and b"deterministic" in err()
        assert L.crl_car_policy_set_sampling(None, 0, flag) == -1 and b"deterministic" in err()
    assert L.crl_car_policy_set_weights(None, 0, blob, 1, None) == -1 and b"null" in err()
    assert L.crl_car_policy_get_weights(None, 0, None, None, None) == -1 and b"null" in err()
    assert L.crl_car_policy_set_sampling(None, 0, 0) == -1 and b"null" in err()
    assert L.crl_car_policy_set_assignment(None, None, None) == -1 and L.crl_car_policy_get_assignment(None, None, None) == -1
    assert L.crl_car_policy_act(None, None, None, None, None, None, None) == -1 and b"null" in err()
    assert L.crl_car_policy_observe(None, None, None) == -1 and b"null" in err()
    assert L.crl_car_policy_get_counters(None, None, None) == -1
    assert L.crl_car_policy_set_counters(None, 0, -1) == -1 and b"calls" in err()
    assert L.crl_car_policy_set_counters(None, 0, 1 << 32) == -1 and L.crl_car_policy_set_counters(None, 0, 0) == -1
    L.crl_car_policy_destroy(None)
    assert (N.CRL_CAR_POLICY_SLOTS, N.CRL_CAR_OBS_FEATURES, N.CRL_CAR_POLICY_BLOB_FLOATS) == (8, 21, 2508)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "crl.h")).read()
    for name in ("CRL_CAR_POLICY_SLOTS 8", "CRL_CAR_OBS_FEATURES 21", "CRL_CAR_POLICY_BLOB_FLOATS 2508", "CRL_CAR_POLICY_DOMAIN 0x43525030u"):
        assert "#define " + name in hdr, name
    assert float(R.CAR_POLICY_TWO_PI).hex() == "0x1.921fb60000000p+2" and "CRL_CAR_POLICY_TWO_PI 0x1.921fb6p+2f" in hdr
    assert float(R.CAR_POLICY_LN_2PI).hex() == "0x1.d67f1c0000000p+0" and "CRL_CAR_POLICY_LN_2PI 0x1.d67f1cp+0f" in hdr
