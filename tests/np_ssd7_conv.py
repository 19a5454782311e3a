"""Float64 NumPy statement of SSD7's trunk convolutions and their gradients (csrc/ssdhip_convbn.hip with the bias epilogue,
csrc/ssdhip_wgrad7.hip): Conv2D(k, 'same', stride 1) for k in {3, 5} as k x k shifted multiply-adds over a zero-padded array -- no
library convolution, nothing of the package.  Maps are NHWC arrays [B, H, W, C], filters [Cout, k, k, Cin] (the memory order of a
channels_last (Cout, Cin, k, k) tensor).  tests/np_conv_grads.py stops at k = 3; its tap view, channel sums and rounding rule are
reused.  tests/test_ssd7_conv_reference_cpu.py pins this module to torch's CPU float64 autograd of F.conv2d."""
import numpy as np

from tests.np_conv_grads import _tap, channel_sums, to_bf16  # noqa: F401

# (kernel, Cin, Cout) of the seven layers, and their maps for the 300 x 480 images of ssd7_training.ipynb
LAYERS = [(5, 3, 32), (3, 32, 48), (3, 48, 64), (3, 64, 64), (3, 64, 48), (3, 48, 48), (3, 48, 32)]
MAPS_300x480 = [(300, 480), (150, 240), (75, 120), (37, 60), (18, 30), (9, 15), (4, 7)]


def _padded(x, pad):
    b, h, w, c = x.shape
    out = np.zeros((b, h + 2 * pad, w + 2 * pad, c))
    out[:, pad:pad + h, pad:pad + w] = x
    return out


def conv_same(x, w, bias=None):
    """y [B, H, W, Cout] = sum_{kh, kw} x_padded[b, h + kh, w + kw, :] . w[co, kh, kw, :] (+ bias[co])."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    b, h, wd, _ = x.shape
    cout, k = w.shape[0], w.shape[1]
    padded = _padded(x, k // 2)
    y = np.zeros((b, h, wd, cout))
    for kh in range(k):
        for kw in range(k):
            y += _tap(padded, kh, kw, h, wd, 1, 1) @ w[:, kh, kw, :].T
    return y if bias is None else y + np.asarray(bias, dtype=np.float64)


def conv_same_input_grad(dy, w):
    """dL/dx [B, H, W, Cin]: dx_padded[b, h + kh, w + kw, ci] += sum_co dy[b, h, w, co] w[co, kh, kw, ci]; the padding is cut."""
    dy, w = np.asarray(dy, dtype=np.float64), np.asarray(w, dtype=np.float64)
    b, h, wd, _ = dy.shape
    k, cin, pad = w.shape[1], w.shape[3], w.shape[1] // 2
    padded = np.zeros((b, h + 2 * pad, wd + 2 * pad, cin))
    for kh in range(k):
        for kw in range(k):
            _tap(padded, kh, kw, h, wd, 1, 1)[...] += dy @ w[:, kh, kw, :]
    return padded[:, pad:pad + h, pad:pad + wd]


def conv_same_weight_grad(x, dy, k):
    """(dw [Cout, k, k, Cin], db [Cout]): dw[co, kh, kw, ci] = sum_{b, h, w} dy[b, h, w, co] x_padded[b, h + kh, w + kw, ci]."""
    x, dy = np.asarray(x, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    b, h, wd, cin = x.shape
    cout = dy.shape[3]
    padded = _padded(x, k // 2)
    flat = dy.reshape(-1, cout).T
    dw = np.zeros((cout, k, k, cin))
    for kh in range(k):
        for kw in range(k):
            dw[:, kh, kw, :] = flat @ _tap(padded, kh, kw, h, wd, 1, 1).reshape(-1, cin)
    return dw, channel_sums(dy)


def flipped(w):
    """The data gradient's filters [Cin, k, k, Cout]: taps flipped, channels swapped (w.flip(2, 3).transpose(0, 1) of the torch tensor)."""
    return np.ascontiguousarray(np.asarray(w)[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))
