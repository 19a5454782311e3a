"""Float64 NumPy statement of the prediction assembly (csrc/ssdhip_heads.h, head_build_rows: what head_kernel writes and
scan_heads_kernel decodes) and of its backward (csrc/ssdhip_layers.hip, head_grad_kernel), written from the definition -- the
graph's Reshape((-1, C)) + Concatenate(axis=1) + Activation('softmax') + AnchorBoxes + Concatenate(axis=2),
models/keras_ssd300.py:363-419 -- and not from the kernel's loops: no tiles, no strides walked with carries, no staging.

Maps are NHWC arrays [B, h, w, channels]; anchor a of a map is (y, x, box) row-major, as the Reshape reads the convolution's output.
Layer i is given either as two dense arrays confs[i] [B, h, w, n_boxes C] and locs[i] [B, h, w, n_boxes 4], or -- locs[i] is None --
as one packed array whose channels are [conf n_boxes C | loc n_boxes 4 | padding]; padding is never read.

tests/test_head_reference_cpu.py pins this module to torch's CPU float64 softmax and autograd and to a hand-computed case."""
import numpy as np


def bf16_round(x):
    """Round float64 values ONCE to bfloat16 (8 significant bits, round to nearest even), returned as float64.  Non-finite values pass."""
    x = np.asarray(x, dtype=np.float64)
    out = x.copy()
    fin = np.isfinite(x) & (x != 0)
    _, e = np.frexp(x[fin])                                   # |x| = m 2^e, m in [0.5, 1): the quantum of 8 significant bits is 2^(e-8)
    q = np.ldexp(1.0, np.maximum(e - 8, -133))                # (bf16 subnormals: multiples of 2^-133)
    r = np.rint(x[fin] / q) * q                               # rint: ties to even
    r[np.abs(r) >= 2.0 ** 128] = np.inf * np.sign(r[np.abs(r) >= 2.0 ** 128])
    out[fin] = r
    return out


def is_bf16(x):
    x = np.asarray(x, dtype=np.float64)
    return bool(np.array_equal(bf16_round(x), x, equal_nan=True))


def softmax(z):
    """Over the last axis, float64.  A NaN makes its whole row NaN; -inf among finite values gives exactly 0."""
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(z - np.max(z, axis=-1, keepdims=True))
        return e / np.sum(e, axis=-1, keepdims=True)


def split_layer(conf, loc, n_boxes, C):
    """(logits [B, h w n_boxes, C], offsets [B, h w n_boxes, 4]) of one layer in either layout."""
    conf = np.asarray(conf, dtype=np.float64)
    b, h, w, ch = conf.shape
    if loc is None:
        assert ch >= n_boxes * (C + 4), "packed map too narrow"
        loc = conf[..., n_boxes * C:n_boxes * (C + 4)]
        conf = conf[..., :n_boxes * C]
    else:
        loc = np.asarray(loc, dtype=np.float64)
        assert ch == n_boxes * C and loc.shape == (b, h, w, n_boxes * 4)
    return conf.reshape(b, h * w * n_boxes, C), loc.reshape(b, h * w * n_boxes, 4)


def assemble(confs, locs, conf_biases, loc_biases, n_boxes, anchors_var, C, src="bf16"):
    """y_pred (B, N, C + 12) float64 = [softmax(conf + bias) | loc + bias | anchor | variances].

    src="bf16": the head outputs and biases are bf16 numbers; conf + bias and loc + bias are each rounded once to bf16 before the
    softmax (the framework's bf16 bias add, which the kernel keeps).  src="f32": the float32 head outputs carry their bias already:
    no bias, no rounding."""
    assert src in ("bf16", "f32")
    zs, ls = [], []
    for i, nb in enumerate(n_boxes):
        z, lo = split_layer(confs[i], locs[i], nb, C)
        cb = conf_biases[i] if conf_biases is not None else None
        lb = loc_biases[i] if loc_biases is not None else None
        if src == "f32":
            assert cb is None and lb is None
        else:
            if cb is not None:                                 # bias [n_boxes C]: entry (box, class); anchor a has box a % n_boxes
                z = bf16_round(z.reshape(z.shape[0], -1, nb, C) + np.asarray(cb, dtype=np.float64).reshape(nb, C)).reshape(z.shape)
            if lb is not None:
                lo = bf16_round(lo.reshape(lo.shape[0], -1, nb, 4) + np.asarray(lb, dtype=np.float64).reshape(nb, 4)).reshape(lo.shape)
        zs.append(z)
        ls.append(lo)
    z, lo = np.concatenate(zs, axis=1), np.concatenate(ls, axis=1)
    av = np.asarray(anchors_var, dtype=np.float64)
    assert av.shape == (z.shape[1], 8)
    return np.concatenate([softmax(z), lo, np.broadcast_to(av, (z.shape[0],) + av.shape)], axis=2)


def assemble_backward(grad_pred, y_pred, n_boxes, strides, C, maps):
    """The packed gradients, one [B, h, w, strides[i]] float64 array per layer of `maps` [(h, w)]: class columns
    dlogit_c = p_c (g_c - sum_k g_k p_k) with p the probabilities of y_pred, offset columns passed through, the anchor and
    variance columns have no producer, padding channels zero."""
    g, y = np.asarray(grad_pred, dtype=np.float64), np.asarray(y_pred, dtype=np.float64)
    assert g.shape == y.shape and g.shape[2] == C + 12
    B = g.shape[0]
    p, gc = y[..., :C], g[..., :C]
    dz = p * (gc - np.sum(gc * p, axis=-1, keepdims=True))
    outs, off = [], 0
    for nb, st, (h, w) in zip(n_boxes, strides, maps):
        n = h * w * nb
        assert st >= nb * (C + 4)
        out = np.zeros((B, h, w, st))
        out[..., :nb * C] = dz[:, off:off + n].reshape(B, h, w, nb * C)
        out[..., nb * C:nb * (C + 4)] = g[:, off:off + n, C:C + 4].reshape(B, h, w, nb * 4)
        outs.append(out)
        off += n
    assert off == g.shape[1]
    return outs


SOFTMAX_ABS = 2e-6                     # the project's bar on assembled class probabilities (tests/test_layers_gpu.py)


def softmax_rel(C):
    """Relative bound of a float32 softmax over C logits with |logit| <= 16 against the exact one, in units of the exact value:
    expf to two ulp, the rounding of x - max (at most 32 2^-24 after expf), C - 1 roundings of the sequential sum, one division."""
    return (C + 40) * 2.0 ** -24


def compare_rows(got, want, C):
    """THE comparison of assembled rows: `got` float32 (..., C + 12) from the GPU, `want` float64 from `assemble`.
    Offset, anchor and variance columns bit for bit; class columns within softmax_rel(C) of the exact value AND within 2e-6;
    NaN exactly where the reference has NaN.  Raises AssertionError naming the first offending entry."""
    got = np.asarray(got)
    want = np.asarray(want, dtype=np.float64)
    assert got.dtype == np.float32, got.dtype
    assert got.shape == want.shape and got.shape[-1] == C + 12, (got.shape, want.shape)
    tail_w = want[..., C:].astype(np.float32)
    assert np.array_equal(tail_w.astype(np.float64), want[..., C:], equal_nan=True), "the reference's offsets / anchors are not float32 numbers"
    bad = np.ascontiguousarray(got[..., C:]).view(np.uint32) != np.ascontiguousarray(tail_w).view(np.uint32)
    bad &= ~(np.isnan(got[..., C:]) & np.isnan(tail_w))
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError("offset / anchor / variance column differs at %s (column C + %d): got %r, want %r (%d entries differ)"
                             % (i[:-1], i[-1], got[..., C:][i], tail_w[i], int(bad.sum())))
    gp, wp = got[..., :C].astype(np.float64), want[..., :C]
    nan_g, nan_w = np.isnan(gp), np.isnan(wp)
    if not np.array_equal(nan_g, nan_w):
        i = tuple(int(v[0]) for v in np.nonzero(nan_g != nan_w))
        raise AssertionError("NaN mismatch at %s: got %r, want %r" % (i, gp[i], wp[i]))
    err = np.where(nan_w, 0.0, np.abs(gp - wp))
    bound = np.minimum(softmax_rel(C) * np.where(nan_w, 0.0, wp), SOFTMAX_ABS)
    bad = err > bound
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        raise AssertionError("class probability at %s: got %r, want %r, error %.3g > %.3g (%d entries beyond the bound)"
                             % (i, gp[i], wp[i], err[i], bound[i], int(bad.sum())))
    return float(np.max(np.where(wp > 0, err / np.where(wp > 0, wp, 1.0), 0.0))) if wp.size else 0.0
