"""What the ``state_dict()`` / ``load_state_dict()`` pairs of ``Policy``, ``AgentPool`` / ``LeagueEnvWrapper`` / ``LeagueArena``,
``RolloutStorage`` and ``LightPPO`` / ``FullPPO`` share (include/crl.h "checkpoint / resume"): the layouts of the weight blobs the
device holds, their cut into torch-layout arrays and back, and the host-side checks a load makes BEFORE it writes anything.

Pure numpy: nothing here touches the GPU.  A refused load raises a ``ValueError`` whose text starts with ``load_state_dict``.

The reference's trainers save ``model.state_dict()`` and the optimiser's with ``torch.save``; the dicts here are their counterpart for
the objects that live on the device: plain dicts of numpy arrays, Python scalars, strings and nested dicts of those.
"""
import collections

import numpy as np

# the policy blob of csrc/pong_league.h with its critic tail: offset and shape of each tensor, 8 488 floats with the pads
BLOB_FLOATS = 8488
BLOB_LAYOUT = collections.OrderedDict((("conv1_w", (0, (16, 4, 4, 4))), ("conv1_b", (1024, (16,))), ("conv2_w", (1040, (16, 16, 2, 2))),
                                       ("conv2_b", (2064, (16,))), ("actor_w", (2080, (3, 1600))), ("actor_b", (6880, (3,))),
                                       ("critic_w", (6884, (1, 1600))), ("critic_b", (8484, (1,)))))
# the blob of a full-size crl_policy (csrc/pong_policy_full.hip) with its critic tail: 1 001 784 floats with the pads
FULL_BLOB_FLOATS = 1001784
FULL_BLOB_LAYOUT = collections.OrderedDict((("conv1_w", (0, (16, 4, 4, 4))), ("conv1_b", (1024, (16,))), ("conv2_w", (1040, (32, 16, 4, 4))),
                                            ("conv2_b", (9232, (32,))), ("conv3_w", (9264, (256, 32, 11, 11))), ("conv3_b", (1000496, (256,))),
                                            ("actor_w", (1000752, (3, 256))), ("actor_b", (1001520, (3,))), ("critic_w", (1001524, (1, 256))),
                                            ("critic_b", (1001780, (1,)))))
CRITIC_KEYS = ("critic_w", "critic_b")
# a pool slot's blob ends in front of the critic
SLOT_FLOATS, FULL_SLOT_FLOATS = BLOB_LAYOUT["critic_w"][0], FULL_BLOB_LAYOUT["critic_w"][0]
NETWORKS = {True: "light", False: "full"}  # [use_light_model]


def layout_of(light, critic=True):
    """(layout, floats) of a network's blob: with the critic tail (a policy's, a learner's) or without it (a pool slot's)."""
    layout, floats = (BLOB_LAYOUT, BLOB_FLOATS) if light else (FULL_BLOB_LAYOUT, FULL_BLOB_FLOATS)
    if critic:
        return layout, floats
    cut = collections.OrderedDict((k, v) for k, v in layout.items() if k not in CRITIC_KEYS)
    return cut, (SLOT_FLOATS if light else FULL_SLOT_FLOATS)


def split_blob(blob, layout):
    """The tensors of a flat float32 blob as arrays of their own (copies), by key, in torch layout; the pads are dropped."""
    blob = np.asarray(blob, np.float32).reshape(-1)
    return {k: blob[o:o + int(np.prod(s))].reshape(s).copy() for k, (o, s) in layout.items()}


def refuse(text):
    return ValueError("load_state_dict: " + text)


def join_blob(arrays, layout, floats, what="weights"):
    """The flat float32 blob of ``floats`` floats from a dict of arrays (pads zero).  A missing key or a wrong shape is refused."""
    blob = np.zeros(int(floats), np.float32)
    for k, (o, s) in layout.items():
        if not isinstance(arrays, dict) or k not in arrays:
            raise refuse(f"{what}: {k} is missing")
        a = np.asarray(arrays[k])
        if tuple(a.shape) != tuple(s):
            raise refuse(f"{what}: {k} has shape {tuple(a.shape)}, this network's is {tuple(s)}")
        blob[o:o + a.size] = np.ascontiguousarray(a, np.float32).reshape(-1)
    return blob


def check_header(sd, kind, what, **sizes):
    """``sd`` is a dict of kind ``kind`` whose sizes are this object's (``sizes``: key -> the object's value)."""
    if not isinstance(sd, dict) or sd.get("kind") != kind:
        raise refuse(f"a state dict of kind {kind!r} is needed for {what}, not {sd.get('kind') if isinstance(sd, dict) else type(sd).__name__!r}")
    for k, mine in sizes.items():
        if k not in sd or sd[k] != mine:
            raise refuse(f"{what}: {k} is {sd.get(k)!r} in the state dict and {mine!r} here")


def check_array(sd, key, shape, itemsize, what):
    """``sd[key]`` as a contiguous array of ``shape`` whose elements have ``itemsize`` bytes (the caller names the dtype it views it as)."""
    if key not in sd or sd[key] is None:
        raise refuse(f"{what}: {key} is missing")
    a = np.ascontiguousarray(sd[key])
    if tuple(a.shape) != tuple(shape) or a.dtype.itemsize != itemsize:
        raise refuse(f"{what}: {key} has shape {tuple(a.shape)} and {a.dtype.itemsize}-byte elements, needed are {tuple(shape)} and {itemsize}")
    return a


def check_counter(value, bits, name, what):
    """A Python int in [0, 2^bits)."""
    try:
        v = int(value)
    except (TypeError, ValueError):
        raise refuse(f"{what}: {name} must be an integer, not {value!r}") from None
    if not 0 <= v < 2 ** bits:
        raise refuse(f"{what}: {name} = {v} lies outside [0, 2^{bits})")
    return v


def check_style(temperature, epsilon, what):
    """(temperature, epsilon) as ``rules.check_sampling`` accepts them, refused in a load's words otherwise."""
    from .rules import check_sampling

    try:
        return check_sampling(temperature, epsilon)
    except (ValueError, TypeError) as e:
        raise refuse(f"{what}: {e}") from None


def nbytes(sd):
    """Bytes of the arrays in a state dict (nested dicts and lists included); scalars and strings count 0."""
    if isinstance(sd, np.ndarray):
        return int(sd.nbytes)
    if isinstance(sd, dict):
        return sum(nbytes(v) for v in sd.values())
    if isinstance(sd, (list, tuple)):
        return sum(nbytes(v) for v in sd)
    return 0
