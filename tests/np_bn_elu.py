"""Float64 NumPy statement of what csrc/ssdhip_bntrain.hip computes: BatchNormalization with batch statistics -> ELU(alpha=1)
[-> MaxPooling2D(2, 2) 'valid'] forward and backward on NHWC maps, the pool winner rule included.  Inputs are float64 arrays holding
bf16-representable values (what the kernels read); nothing here is rounded.  tests/test_bn_elu_train_cpu.py pins it to torch's CPU
autograd; the GPU tests compare the kernels with it."""
import numpy as np


def batch_stats(y):
    """(mean, biased variance, unbiased variance) per channel of y [B, H, W, C]: two passes, no E[y^2] - mean^2."""
    m = y.shape[0] * y.shape[1] * y.shape[2]
    flat = y.reshape(m, -1)
    mean = flat.sum(axis=0) / m
    m2 = ((flat - mean) ** 2).sum(axis=0)
    return mean, m2 / m, m2 / (m - 1)


def running_update(running, stat, momentum):
    """nn.BatchNorm2d's rule (for running_var `stat` is the UNBIASED variance)."""
    return (1.0 - momentum) * running + momentum * stat


def elu(v):
    return np.where(v > 0, v, np.expm1(np.minimum(v, 0)))


def winners(y, gamma):
    """Boolean [B, H, W, C]: the position wins its 2 x 2 window.  The winner is the first position in the order (0,0), (0,1), (1,0),
    (1,1) among those with the largest s y, s = +1 for gamma >= 0 and -1 otherwise; for gamma = 0 it is (0,0).  The odd last row /
    column belongs to no window."""
    b, h, w, c = y.shape
    ho, wo = h // 2, w // 2
    win = np.zeros(y.shape, dtype=bool)
    if ho == 0 or wo == 0:
        return win
    s = np.where(gamma >= 0, 1.0, -1.0)
    key = (y * s)[:, :2 * ho, :2 * wo].reshape(b, ho, 2, wo, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(b, ho, wo, 4, c)
    key = np.where(gamma == 0, 0.0, key)                  # every position ties: argmax takes the first
    first = np.argmax(key, axis=3)                        # argmax returns the FIRST maximum
    onehot = first[:, :, :, None, :] == np.arange(4)[None, None, None, :, None]
    win[:, :2 * ho, :2 * wo] = onehot.reshape(b, ho, wo, 2, 2, c).transpose(0, 1, 3, 2, 4, 5).reshape(b, 2 * ho, 2 * wo, c)
    return win


def forward(y, gamma, beta, eps):
    """-> dict(mean, var, var_unbiased, invstd, full, pooled): full = elu(y scale + shift) [B, H, W, C], pooled its 2 x 2 'valid'
    maximum [B, H // 2, W // 2, C] (None for a map without a window)."""
    b, h, w, c = y.shape
    mean, var, var_u = batch_stats(y)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * invstd
    full = elu(y * scale + (beta - mean * scale))
    ho, wo = h // 2, w // 2
    pooled = None
    if ho and wo:
        pooled = full[:, :2 * ho, :2 * wo].reshape(b, ho, 2, wo, 2, c).max(axis=(2, 4))
    return dict(mean=mean, var=var, var_unbiased=var_u, invstd=invstd, full=full, pooled=pooled)


def backward(y, gamma, beta, eps, g_full=None, g_pooled=None):
    """-> (dy, dgamma, dbeta, routed): g_e = g_full + [position wins] g_pooled (`routed` is that mask times g_pooled spread over the
    full map); dv = g_e (v > 0 ? 1 : exp(v)); dbeta = sum dv; dgamma = sum dv xhat; dy = gamma invstd (dv - dbeta / M - xhat dgamma / M)."""
    b, h, w, c = y.shape
    m = b * h * w
    mean, var, _ = batch_stats(y)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * invstd
    v = y * scale + (beta - mean * scale)
    g = np.zeros(y.shape) if g_full is None else g_full.astype(np.float64).copy()
    routed = np.zeros(y.shape)
    if g_pooled is not None:
        ho, wo = h // 2, w // 2
        spread = np.repeat(np.repeat(g_pooled, 2, axis=1), 2, axis=2)
        routed[:, :2 * ho, :2 * wo] = spread
        routed *= winners(y, gamma)
        g = g + routed
    dv = g * np.where(v > 0, 1.0, np.exp(np.minimum(v, 0)))
    xhat = (y - mean) * invstd
    dbeta = dv.reshape(m, c).sum(axis=0)
    dgamma = (dv * xhat).reshape(m, c).sum(axis=0)
    dy = scale * (dv - dbeta / m - xhat * dgamma / m)
    return dy, dgamma, dbeta, routed


def to_bf16(a):
    """float array -> the nearest bf16 values (round to nearest even), as float64."""
    u = np.asarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32).astype(np.float64)


def bf16_step(a):
    """The spacing of bf16 numbers at |a| (8 significant bits), at least the smallest normal's."""
    a = np.maximum(np.abs(np.asarray(a, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)
