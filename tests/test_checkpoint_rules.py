"""The host side of checkpoint / resume (competitive_rl_amd/checkpoint.py): the blob layouts against the shapes the loaders check, the
cut of a blob into torch-layout arrays and back, and what a load refuses before it writes anything.  No GPU."""
import io

import numpy as np
import pytest

from competitive_rl_amd import checkpoint as K
from competitive_rl_amd import ppo
from competitive_rl_amd.policy_serving import _CRITIC_SHAPES, _FULL_SHAPES, _SHAPES
from competitive_rl_amd.rules import PPO_FULL_KEYS, PPO_KEYS


@pytest.mark.parametrize("light", [True, False])
def test_the_layouts_are_the_networks_tensors_back_to_back_with_zero_pads(light):
    layout, floats = K.layout_of(light)
    shapes = dict(_SHAPES if light else _FULL_SHAPES, **_CRITIC_SHAPES[light])
    assert tuple(layout) == (PPO_KEYS if light else PPO_FULL_KEYS) and {k: s for k, (_, s) in layout.items()} == shapes
    assert floats == (8488 if light else 1001784) and floats % 4 == 0
    end = 0
    for k, (o, s) in layout.items():
        assert end <= o <= end + 3 and o % 4 == 0, k  # (each tensor starts at the next multiple of four floats)
        end = o + int(np.prod(s))
    assert end <= floats <= end + 3
    slot, slot_floats = K.layout_of(light, critic=False)
    assert tuple(slot) == tuple(layout)[:-2] and slot_floats == layout["critic_w"][0] == (6884 if light else 1001524)
    assert ppo.BLOB_LAYOUT is K.BLOB_LAYOUT and ppo.FULL_BLOB_LAYOUT is K.FULL_BLOB_LAYOUT and ppo.BLOB_FLOATS == 8488  # (where they lived before)


@pytest.mark.parametrize("light", [True, False])
def test_split_and_join_are_inverse_and_the_pads_stay_zero(light):
    layout, floats = K.layout_of(light)
    rs = np.random.RandomState(1)
    w = {k: rs.standard_normal(s).astype(np.float32) for k, (_, s) in layout.items()}
    blob = K.join_blob(w, layout, floats)
    assert blob.dtype == np.float32 and blob.shape == (floats,)
    used = np.zeros(floats, bool)
    for o, s in layout.values():
        used[o:o + int(np.prod(s))] = True
    assert not blob[~used].any() and (~used).sum() == floats - sum(int(np.prod(s)) for _, s in layout.values())
    back = K.split_blob(blob, layout)
    assert all(back[k].tobytes() == w[k].tobytes() and back[k].shape == w[k].shape for k in w)
    back["conv1_b"][0] += 1
    assert blob[layout["conv1_b"][0]] == w["conv1_b"][0]  # (copies, not views)


def test_what_a_load_refuses_says_load_state_dict():
    layout, floats = K.layout_of(True)
    w = {k: np.zeros(s, np.float32) for k, (_, s) in layout.items()}
    for bad in ({k: v for k, v in w.items() if k != "actor_b"}, dict(w, conv1_w=np.zeros((16, 4, 4, 3), np.float32)), None):
        with pytest.raises(ValueError, match="load_state_dict"):
            K.join_blob(bad, layout, floats)
    sd = {"kind": "Policy", "num_envs": 4, "names": ["A", "B"], "x": np.zeros((4, 2), np.int32)}
    K.check_header(sd, "Policy", "Policy", num_envs=4, names=["A", "B"])
    for kind, sizes in (("LightPPO", {}), ("Policy", {"num_envs": 5}), ("Policy", {"names": ["B", "A"]}), ("Policy", {"rows": 4})):
        with pytest.raises(ValueError, match="load_state_dict"):
            K.check_header(sd, kind, "Policy", **sizes)
    with pytest.raises(ValueError, match="load_state_dict"):
        K.check_header([1, 2], "Policy", "Policy")
    assert K.check_array(sd, "x", (4, 2), 4, "t") is not None
    for key, shape, size in (("x", (4, 3), 4), ("x", (4, 2), 1), ("y", (4, 2), 4)):
        with pytest.raises(ValueError, match="load_state_dict"):
            K.check_array(sd, key, shape, size, "t")
    assert K.check_counter(np.int64(7), 32, "n", "t") == 7 and K.check_counter(2 ** 64 - 1, 64, "n", "t") == 2 ** 64 - 1
    for v, bits in ((-1, 32), (2 ** 32, 32), ("x", 32), (None, 32)):
        with pytest.raises(ValueError, match="load_state_dict"):
            K.check_counter(v, bits, "n", "t")
    assert K.check_style(1.0, 0.1, "t") == (1.0, float(np.float32(0.1)))
    for t, e in ((-1.0, 0.0), (1.0, 1.5), (float("nan"), 0.0)):
        with pytest.raises(ValueError, match="load_state_dict"):
            K.check_style(t, e, "t")


def test_nbytes_counts_the_arrays_of_a_nested_state_dict_and_it_survives_torch_save():
    torch = pytest.importorskip("torch")
    sd = {"kind": "x", "a": np.zeros((3, 4), np.float32), "n": {"b": np.zeros(5, np.uint8), "c": None, "d": [np.zeros(2, np.int64), 3]}, "s": 1.5}
    assert K.nbytes(sd) == 48 + 5 + 16
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=False)
    assert K.nbytes(back) == K.nbytes(sd) and back["n"]["d"][1] == 3 and back["s"] == 1.5
