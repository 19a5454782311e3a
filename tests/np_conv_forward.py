"""Float64 NumPy statement of the inference convolutions (csrc/ssdhip_conv.hip, ssdhip_conv64.hip, ssdhip_convh.hip, ssdhip_convimg.hip,
ssdhip_chain.hip): a convolution is k x k shifted matrix products over a zero-padded array -- no library convolution, nothing of the
package.  Maps are NHWC arrays [B, H, W, C], filters [Cout, k, k, Cin] (the memory order of a channels_last (Cout, Cin, k, k) tensor),
k in {1, 3}.  Inputs hold bf16-representable values; only `chain` rounds (`to_bf16` is tests/np_bn_elu.py's), once per layer.
tests/test_conv_forward_reference_cpu.py pins it to torch's CPU float64 F.conv2d / F.max_pool2d(ceil_mode=True);
tests/test_forward_exact_gpu.py compares the kernels with it."""
import numpy as np

from tests.np_bn_elu import to_bf16  # noqa: F401  (one rounding rule for every reference module)
from tests.np_conv_grads import _tap, out_size  # noqa: F401  (one statement of a tap's view and of the output size)


def conv_forward(x, w, bias, stride, pad, dil):
    """y [B, Ho, Wo, Cout] = bias[co] + sum_{kh, kw, ci} x_padded[b, ho stride + kh dil, wo stride + kw dil, ci] w[co, kh, kw, ci]
    (torch.nn.Conv2d's semantics: `pad` zeros on every side)."""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    b, h, wd, cin = x.shape
    cout, k = w.shape[0], w.shape[1]
    assert w.shape == (cout, k, k, cin) and k in (1, 3)
    ho, wo = out_size(h, stride, pad, dil, k), out_size(wd, stride, pad, dil, k)
    assert ho >= 1 and wo >= 1
    padded = np.zeros((b, h + 2 * pad, wd + 2 * pad, cin))
    padded[:, pad:pad + h, pad:pad + wd] = x
    y = np.zeros((b, ho, wo, cout))
    for kh in range(k):
        for kw in range(k):
            y += _tap(padded, kh, kw, ho, wo, stride, dil) @ w[:, kh, kw, :].T
    if bias is not None:
        y += np.asarray(bias, dtype=np.float64)
    return y


def relu(v):
    return np.maximum(np.asarray(v, dtype=np.float64), 0.0)


def maxpool2_same(v):
    """MaxPooling2D(2, 2, 'same'): [B, (H + 1) // 2, (W + 1) // 2, C], the last window of an odd map clipped to the map."""
    v = np.asarray(v, dtype=np.float64)
    b, h, w, c = v.shape
    full = np.full((b, h + (h & 1), w + (w & 1), c), -np.inf)
    full[:, :h, :w] = v
    return full.reshape(b, (h + 1) // 2, 2, (w + 1) // 2, 2, c).max(axis=(2, 4))


def chain(x, layers):
    """The contract of conv_chain and conv1_block: every layer is convolution (+ bias), then ReLU where the layer has one, then ONE
    rounding to bf16 of the layer's map before the next layer reads it.  `layers`: dicts {w, bias, stride, pad, dil, relu}.
    Returns the list of every layer's EXACT map (before its rounding): the caller rounds the ones it compares."""
    cur, maps = np.asarray(x, dtype=np.float64), []
    for l in layers:
        y = conv_forward(cur, l["w"], l.get("bias"), l.get("stride", 1), l.get("pad", 0), l.get("dil", 1))
        if l.get("relu", True):
            y = relu(y)
        maps.append(y)
        cur = to_bf16(y)
    return maps
