"""CPU restatement of the reference's built-in CNN Pong opponents.  TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this; the product
(competitive_rl_amd) never does.  Pinned to tests/golden/policy_light.npz, which was recorded from
the reference's own Policy / LightActorCritic with the reference's checkpoints
(tests/golden/gen_policy_golden.py).

Follows:
* LightActorCritic.forward (reference utils/network.py:73-93): x/255 -> conv1 4->16 k4 s2 -> ReLU
  -> conv2 16->16 k2 s2 -> ReLU -> flatten (C, H, W order) -> actor_linear (3) / critic_linear (1);
* Policy.__call__ / compute_action (utils/policy_serving.py:46-66): the policy keeps its OWN
  4-frame FrameStackTensor, updated without a mask (never cleared when an episode ends -- the
  reference notes this itself at :38-40), and plays argmax of the logits;
* FrameStackTensor.update (utils/utils.py:159-170): roll by one plane, newest plane last.

float32 throughout; the summation order inside a convolution is not defined by the reference
(torch's CPU convolution), so logits are compared with a tolerance (1e-4 abs) and actions must
agree wherever the two best logits are further apart than that.

forward64 / forward_seq32 restate the same networks in float64 and in float32 with a strictly
sequential summation: with the BLAS-ordered forward / forward_full they are two float32 orders
around one float64 truth, from which tests/policy_f64_cases.py derives the kernels' error budget.
"""
import numpy as np


def load_weights(path):
    z = np.load(path)
    return {k: np.ascontiguousarray(z[k], np.float32) for k in z.files}


def _cols(x, k, stride):
    """im2col of x [B, C, H, W] (valid padding) in torch's k order (ic, ky, kx): [B * Ho * Wo, C * k * k], Ho, Wo."""
    B, C, H, W = x.shape
    Ho, Wo = (H - k) // stride + 1, (W - k) // stride + 1
    cols = np.empty((B, Ho, Wo, C, k, k), x.dtype)
    for ky in range(k):
        for kx in range(k):
            cols[:, :, :, :, ky, kx] = x[:, :, ky:ky + stride * Ho:stride, kx:kx + stride * Wo:stride].transpose(0, 2, 3, 1)
    return cols.reshape(B * Ho * Wo, C * k * k), Ho, Wo


def _conv(x, w, b, stride):
    """x [B, C, H, W] f32, w [O, C, k, k] -> [B, O, H', W'] (valid padding)."""
    O = w.shape[0]
    cols, Ho, Wo = _cols(x.astype(np.float32, copy=False), w.shape[2], stride)
    y = cols @ w.reshape(O, -1).T + b
    return y.reshape(x.shape[0], Ho, Wo, O).transpose(0, 3, 1, 2).astype(np.float32)


def forward(wts, stack_u8):
    """stack_u8 [B, 4, 42, 42] (oldest plane first) -> (logits [B, 3], value [B]) float32."""
    x = np.asarray(stack_u8).astype(np.float32) / np.float32(255.0)
    h = np.maximum(_conv(x, wts["conv1_w"], wts["conv1_b"], 2), 0)
    h = np.maximum(_conv(h, wts["conv2_w"], wts["conv2_b"], 2), 0)
    f = h.reshape(h.shape[0], -1)
    logits = f @ wts["actor_w"].T + wts["actor_b"]
    value = f @ wts["critic_w"].T + wts["critic_b"]
    return logits.astype(np.float32), value.reshape(-1).astype(np.float32)


def forward_full(wts, stack_u8):
    """ActorCritic.forward (reference utils/network.py:14-50) on stacks [B, 4, 42, 42]: x/255 -> conv1 4->16 k4 s2 -> ReLU -> conv2
    16->32 k4 s2 pad 2 -> ReLU -> conv3 32->256 k11 -> ReLU -> flatten (256) -> actor_linear (3) / critic_linear (1)."""
    x = np.asarray(stack_u8).astype(np.float32) / np.float32(255.0)
    h = np.maximum(_conv(x, wts["conv1_w"], wts["conv1_b"], 2), 0)            # [B, 16, 20, 20]
    h = np.pad(h, ((0, 0), (0, 0), (2, 2), (2, 2)))
    h = np.maximum(_conv(h, wts["conv2_w"], wts["conv2_b"], 2), 0)            # [B, 32, 11, 11]
    h = np.maximum(_conv(h, wts["conv3_w"], wts["conv3_b"], 1), 0)            # [B, 256, 1, 1]
    f = h.reshape(h.shape[0], -1)
    logits = f @ wts["actor_w"].T + wts["actor_b"]
    value = f @ wts["critic_w"].T + wts["critic_b"]
    return logits.astype(np.float32), value.reshape(-1).astype(np.float32)


# ---- two more statements of the same networks, around which the device kernels' logits are budgeted (tests/policy_f64_cases.py):
# forward64 is the truth, forward_seq32 a second float32 summation order beside BLAS's (forward / forward_full above)
def _dot64(a, w, b):
    return a @ w.T + b


def _dot_seq32(a, w, b):
    """bias first, then one product after the other in k order, every product and every sum rounded to float32"""
    at, wt = np.ascontiguousarray(a.T), np.ascontiguousarray(w.T)  # [K, M], [K, O]
    acc = np.broadcast_to(b.astype(np.float32), (a.shape[0], w.shape[0])).copy()
    for k in range(at.shape[0]):
        acc += at[k][:, None] * wt[k][None, :]
    return acc


def network(wts, stack_u8, full, dtype, dot, operands=None):
    """Both networks layer by layer in `dtype`; `dot(a [M, K], w [O, K], b [O]) -> [M, O]` is the one place where sums are formed.
    `operands(layer, a, w) -> (a, w)` may replace a layer's operands (the tests' fault models); the references pass None."""
    x = np.asarray(stack_u8).astype(dtype) / dtype(255.0)
    layers = (("conv1", 2, 0), ("conv2", 2, 2), ("conv3", 1, 0)) if full else (("conv1", 2, 0), ("conv2", 2, 0))
    for name, stride, pad in layers:
        w = wts[name + "_w"]
        if pad:
            x = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)))
        a, Ho, Wo = _cols(x, w.shape[2], stride)
        wm = w.reshape(w.shape[0], -1).astype(dtype)
        if operands is not None:
            a, wm = operands(name, a, wm)
        y = dot(a, wm, wts[name + "_b"].astype(dtype))
        x = np.maximum(y.reshape(x.shape[0], Ho, Wo, w.shape[0]).transpose(0, 3, 1, 2), 0)
    f = x.reshape(x.shape[0], -1)
    logits = dot(f, wts["actor_w"].astype(dtype), wts["actor_b"].astype(dtype))
    value = dot(f, wts["critic_w"].astype(dtype), wts["critic_b"].astype(dtype)).reshape(-1) if "critic_w" in wts else None
    return logits, value


def forward64(wts, stack_u8, full=False):
    """The same network in plain float64: x / 255.0 in float64, the float32 weights widened.  (logits [B, 3], value [B] or None when
    the weight set has no critic) float64."""
    return network(wts, stack_u8, full, np.float64, _dot64)


def forward_seq32(wts, stack_u8, full=False):
    """float32 throughout, every dot product accumulated strictly one term at a time in torch's k order (ic, ky, kx), bias first, each
    product and each sum rounded to float32: a second float32 summation order beside BLAS's."""
    return network(wts, stack_u8, full, np.float32, _dot_seq32)


class PolicyOracle:
    """Policy(…, use_light_model=True) of utils/policy_serving.py as a callable on (N, 1, 42, 42) frames."""

    def __init__(self, weights, num_envs, dtype=np.uint8, full=False):
        self.w = weights
        self.fwd = forward_full if full else forward  # full: ActorCritic (STRONG / ALPHA_PONG's model) instead of LightActorCritic
        self.stack = np.zeros((num_envs, 4, 42, 42), dtype)  # (float32: the frames of the reference's unrounded float32 step path)
        self.logits = None

    def reset(self):
        self.stack[:] = 0

    def __call__(self, obs):
        obs = np.asarray(obs).reshape(self.stack.shape[0], 42, 42)
        self.stack = np.roll(self.stack, -1, axis=1)
        self.stack[:, -1] = obs
        self.logits, self.value = self.fwd(self.w, self.stack)
        return self.logits.argmax(1).reshape(-1, 1)
