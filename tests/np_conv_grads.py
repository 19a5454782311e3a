"""Float64 NumPy statement of the backward operations of the VGG / SSD300 training step (csrc/ssdhip_wgrad.hip, csrc/ssdhip_train.hip
and the data gradient through the forward kernels): each convolution gradient is k x k shifted multiply-adds over a zero-padded
array -- no library convolution, nothing of the package.  Maps are NHWC arrays [B, H, W, C], filters [Cout, k, k, Cin] (the memory
order of a channels_last (Cout, Cin, k, k) tensor), k in {1, 3}.  Inputs hold bf16-representable values; nothing here is rounded
(`to_bf16` is tests/np_bn_elu.py's).  tests/test_conv_grads_reference_cpu.py pins it to torch's CPU float64 autograd of F.conv2d;
tests/test_backward_exact_gpu.py compares the kernels with it."""
import numpy as np

from tests.np_bn_elu import to_bf16  # noqa: F401  (one rounding rule for both reference modules)


def out_size(n, stride, pad, dil, k):
    """torch.nn.Conv2d's output size along one axis."""
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


def _tap(padded, kh, kw, ho, wo, stride, dil):
    """The view of a zero-padded map that tap (kh, kw) multiplies: padded[:, ho' stride + kh dil, wo' stride + kw dil] for every output."""
    h0, w0 = kh * dil, kw * dil
    return padded[:, h0:h0 + stride * (ho - 1) + 1:stride, w0:w0 + stride * (wo - 1) + 1:stride]


def conv_input_grad(dy, w, x_shape, stride, pad, dil):
    """dL/dx [B, H, W, Cin] of y = conv(x, w) from dy [B, Ho, Wo, Cout] and w [Cout, k, k, Cin]:
    dx_padded[b, ho stride + kh dil, wo stride + kw dil, ci] += sum_co dy[b, ho, wo, co] w[co, kh, kw, ci], then the padding is cut."""
    dy, w = np.asarray(dy, dtype=np.float64), np.asarray(w, dtype=np.float64)
    b, h, wd, cin = x_shape
    cout, k = w.shape[0], w.shape[1]
    ho, wo = out_size(h, stride, pad, dil, k), out_size(wd, stride, pad, dil, k)
    assert dy.shape == (b, ho, wo, cout) and w.shape == (cout, k, k, cin) and k in (1, 3)
    padded = np.zeros((b, h + 2 * pad, wd + 2 * pad, cin))
    for kh in range(k):
        for kw in range(k):
            _tap(padded, kh, kw, ho, wo, stride, dil)[...] += dy @ w[:, kh, kw, :]
    return padded[:, pad:pad + h, pad:pad + wd]


def conv_weight_grad(x, dy, stride, pad, dil, k):
    """dL/dw [Cout, k, k, Cin] of y = conv(x, w) from x [B, H, W, Cin] and dy [B, Ho, Wo, Cout]:
    dw[co, kh, kw, ci] = sum_{b, ho, wo} dy[b, ho, wo, co] x_padded[b, ho stride + kh dil, wo stride + kw dil, ci]."""
    x, dy = np.asarray(x, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    b, h, wd, cin = x.shape
    ho, wo = out_size(h, stride, pad, dil, k), out_size(wd, stride, pad, dil, k)
    cout = dy.shape[3]
    assert dy.shape == (b, ho, wo, cout) and k in (1, 3)
    padded = np.zeros((b, h + 2 * pad, wd + 2 * pad, cin))
    padded[:, pad:pad + h, pad:pad + wd] = x
    dw = np.zeros((cout, k, k, cin))
    flat = dy.reshape(-1, cout).T
    for kh in range(k):
        for kw in range(k):
            dw[:, kh, kw, :] = flat @ _tap(padded, kh, kw, ho, wo, stride, dil).reshape(-1, cin)
    return dw


def relu_mask(g, act):
    """threshold_backward(g, act, 0): the gradient passes where act > 0 (finite activations only)."""
    return np.where(np.asarray(act) > 0, np.asarray(g, dtype=np.float64), 0.0)


def channel_sums(g):
    """[C]: the sum over every pixel of an NHWC map -- a layer's bias gradient."""
    g = np.asarray(g, dtype=np.float64)
    return g.reshape(-1, g.shape[-1]).sum(axis=0)


def embed_strided(dy, h, w, stride, offset):
    """z [B, h, w, C]: zeros with dy[b, i, j] at (offset + stride i, offset + stride j); an entry that falls off the map is dropped."""
    dy = np.asarray(dy, dtype=np.float64)
    b, ho, wo, c = dy.shape
    z = np.zeros((b, h, w, c))
    for i in range(ho):
        for j in range(wo):
            r, s = offset + stride * i, offset + stride * j
            if r < h and s < w:
                z[:, r, s] = dy[:, i, j]
    return z
