"""csrc/ssdhip_bntrain.hip against tests/np_bn_elu.py (float64): batch-statistics BatchNorm -> ELU [-> 2 x 2 'valid' pool] forward
and backward.  Shapes (B, H, W): (1, 1, 2) is M = 2; (2, 1, 1) a map without a window (full form only); (2, 7, 5) odd edges; (3, 2, 2)
one window per image; (3, 37, 35) several partial slots with a ragged last slice.

Tolerances.  Statistics and the two parameter gradients are float32 sums of at most 2^15 terms merged in a fixed tree: the error
is bounded by about (log2 M + 8) 2^-24 ~ 1.4e-6 of the sum of the summands' absolute values, so 1e-5 of that sum leaves 7 x.  A map
value is within one bf16 step of the float64 value plus 1e-5 of its channel's largest magnitude."""
import numpy as np
import pytest

from tests import np_bn_elu as ref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 2), (2, 1, 1), (2, 7, 5), (3, 2, 2), (3, 37, 35)]
FORMS = {"pooled": (True, False), "both": (True, True), "full": (False, True)}
CASES = [(s, c, f) for s in SHAPES for c in (32, 48, 64) for f in FORMS if f == "full" or min(s[1:]) >= 2]


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dtype).cuda()


def _map(a):
    """NHWC float64 array of bf16 values -> (B, C, H, W) bf16 CUDA tensor with NHWC memory."""
    import torch
    return _dev(a, torch.bfloat16).permute(0, 3, 1, 2)


def _np(t):
    """A map (or vector) from the device as float64, maps as NHWC."""
    if t is None:
        return None
    t = t.detach().double().cpu()
    return (t.permute(0, 2, 3, 1) if t.dim() == 4 else t).numpy()


def _params(c, rng, dtype_name):
    """gamma with mixed signs and one exact zero, beta, running buffers: values both dtypes hold exactly."""
    gamma = ref.to_bf16((rng.rand(c) * 0.8 + 0.6) * np.where(rng.rand(c) < 0.4, -1.0, 1.0))
    gamma[3] = 0.0
    return gamma, ref.to_bf16(rng.randn(c) * 0.4), ref.to_bf16(rng.randn(c)), ref.to_bf16(rng.rand(c) + 0.5)


def _random_map(shape, c, rng):
    """|mean| <= 8 std per channel; channel 1 has mean 8 and std 0.25; quantised to bf16."""
    std = rng.rand(c) + 0.5
    mean = (rng.rand(c) * 16 - 8) * std
    mean[1], std[1] = 8.0, 0.25
    return ref.to_bf16(rng.randn(*shape, c) * std + mean)


def _forward(y, gamma, beta, rm, rv, momentum, eps, form, dtype_name):
    import torch
    from ssd_keras_amd import _native as nat
    dt = getattr(torch, dtype_name)
    pool, keep = FORMS[form]
    rmd, rvd = _dev(rm, dt), _dev(rv, dt)
    gd, bd = _dev(gamma, dt), _dev(beta, dt)
    yd = _map(y)
    full, pooled, mean, invstd = nat.bn_elu_train_forward(yd, gd, bd, rmd, rvd, momentum, eps, pool, keep)
    assert (full is None) == (form == "pooled") and (pooled is None) == (form == "full")
    return dict(y=yd, gamma=gd, beta=bd, full=full, pooled=pooled, mean=mean, invstd=invstd, rm=rmd, rv=rvd)


def _backward(run, form, g_full, g_pooled):
    from ssd_keras_amd import _native as nat
    return nat.bn_elu_train_backward(run["y"], run["mean"], run["invstd"], run["gamma"], run["beta"],
                                     None if g_full is None else _map(g_full), None if g_pooled is None else _map(g_pooled))


def _close_map(got, want, what):
    tol = ref.bf16_step(want) + 1e-5 * np.abs(want).max(axis=(0, 1, 2))
    err = np.abs(got - want)
    print("%s: largest error / tolerance %.3g" % (what, float((err / tol).max())))
    assert np.all(err <= tol), what


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
@pytest.mark.parametrize("shape,c,form", CASES)
def test_random_data(shape, c, form, dtype_name):
    from ssd_keras_amd import _native as nat
    b, h, w = shape
    m = b * h * w
    rng = np.random.RandomState(m * 7 + c)
    if shape == (3, 37, 35):
        assert nat.bn_elu_train_blocks(m, c) > 1
    y = _random_map(shape, c, rng)
    gamma, beta, rm, rv = _params(c, rng, dtype_name)
    eps, momentum = 1e-3, 0.25
    run = _forward(y, gamma, beta, rm, rv, momentum, eps, form, dtype_name)
    want = ref.forward(y, gamma, beta, eps)
    sum_abs = np.abs(y).reshape(m, c).sum(axis=0)
    assert np.all(np.abs(_np(run["mean"]) - want["mean"]) <= 1e-5 * sum_abs / m)
    # the variance (every summand is positive: the bound is 1e-5 of itself) through invstd = (var + eps)^-1/2 and through running_var
    assert np.all(np.abs(_np(run["invstd"]) - want["invstd"]) <= 1e-5 * want["invstd"])
    # ... and directly: 1e-5 of the variance, plus what storing invstd in float32 costs (2^-24 of invstd is 2^-23 of var + eps)
    got_var = 1.0 / _np(run["invstd"]) ** 2 - eps
    assert np.all(np.abs(got_var - want["var"]) <= 1e-5 * want["var"] + 2.0 ** -22 * (want["var"] + eps))
    half = (lambda v: 0.5 * ref.bf16_step(v)) if dtype_name == "bfloat16" else (lambda v: 2.0 ** -24 * np.abs(v))
    want_rm = ref.running_update(rm, want["mean"], momentum)
    want_rv = ref.running_update(rv, want["var_unbiased"], momentum)
    assert np.all(np.abs(_np(run["rm"]) - want_rm) <= momentum * 1e-5 * sum_abs / m + half(want_rm) * 1.001)
    assert np.all(np.abs(_np(run["rv"]) - want_rv) <= momentum * 1e-5 * want["var_unbiased"] + half(want_rv) * 1.001)
    if run["full"] is not None:
        _close_map(_np(run["full"]), want["full"], "full")
    if run["pooled"] is not None:
        _close_map(_np(run["pooled"]), want["pooled"], "pooled")
    g_full = ref.to_bf16(rng.randn(b, h, w, c)) if form != "pooled" else None
    g_pooled = ref.to_bf16(rng.randn(b, h // 2, w // 2, c)) if form != "full" else None
    dy, dgamma, dbeta = _backward(run, form, g_full, g_pooled)
    dy_w, dgamma_w, dbeta_w, routed = ref.backward(y, gamma, beta, eps, g_full, g_pooled)
    # the summands of dbeta and dgamma, for the bound
    g = routed + (0 if g_full is None else g_full)
    mean, invstd = want["mean"], want["invstd"]
    v = y * gamma * invstd + (beta - mean * gamma * invstd)
    dv = g * np.where(v > 0, 1.0, np.exp(np.minimum(v, 0)))
    xhat = (y - mean) * invstd
    err_b, tol_b = np.abs(_np(dbeta) - dbeta_w), 1e-5 * np.abs(dv).reshape(m, c).sum(axis=0)
    err_g, tol_g = np.abs(_np(dgamma) - dgamma_w), 1e-5 * np.abs(dv * xhat).reshape(m, c).sum(axis=0)
    print("dbeta err / tol %.3g, dgamma err / tol %.3g" % (float((err_b / np.maximum(tol_b, 1e-300)).max()),
                                                            float((err_g / np.maximum(tol_g, 1e-300)).max())))
    assert np.all(err_b <= tol_b) and np.all(err_g <= tol_g)
    _close_map(_np(dy), dy_w, "dy")


def _exact_map(shape, c, rng):
    """Small integers with per-channel mean m_c (an integer) and biased variance exactly 3 (deviations -3, -1, -1, -1, 1, 1, 1, 3,
    shuffled), or 1 (deviations -1, 1) for M = 2: with eps = 1, or 3, invstd is exactly 1 / 2."""
    b, h, w = shape
    m = b * h * w
    base = np.array([-3, -1, -1, -1, 1, 1, 1, 3], dtype=np.float64) if m % 8 == 0 else np.array([-1.0, 1.0])
    eps = 1.0 if m % 8 == 0 else 3.0
    dev = np.stack([rng.permutation(np.tile(base, m // len(base))) for _ in range(c)], axis=1)
    mean = rng.randint(-4, 5, size=c).astype(np.float64)
    return (dev + mean).reshape(b, h, w, c), mean, eps


@pytest.mark.parametrize("dtype_name", ["float32", "bfloat16"])
@pytest.mark.parametrize("shape", [(1, 1, 2), (2, 4, 4), (4, 16, 32)])
@pytest.mark.parametrize("c", [32, 48, 64])
def test_exact_integer_data(shape, c, dtype_name):
    """M a power of two (2, 32, 2048 -- the last is 16 partial slots): mean, variance, the running update and every positive output
    are the float64 results rounded once; outputs through expm1f are within one bf16 step; the gradient routing is exact."""
    b, h, w = shape
    m = b * h * w
    rng = np.random.RandomState(m + c)
    y, mean, eps = _exact_map(shape, c, rng)
    gamma = rng.choice([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], size=c)
    gamma[3] = 0.0
    beta = rng.randint(-4, 5, size=c) * 0.5
    rm, rv = rng.randint(-3, 4, size=c).astype(np.float64), rng.randint(1, 5, size=c).astype(np.float64)
    momentum = 0.25
    once = (lambda a: ref.to_bf16(np.float32(a))) if dtype_name == "bfloat16" else (lambda a: np.float32(a).astype(np.float64))
    forms = ["full"] if min(h, w) < 2 else ["pooled", "both", "full"]
    for form in forms:
        run = _forward(y, gamma, beta, rm, rv, momentum, eps, form, dtype_name)
        want = ref.forward(y, gamma, beta, eps)
        assert np.array_equal(want["mean"], mean) and np.all(want["invstd"] == 0.5)
        assert np.array_equal(_np(run["mean"]), mean) and np.array_equal(_np(run["invstd"]), want["invstd"])
        assert np.array_equal(_np(run["rm"]), once(ref.running_update(rm, want["mean"], momentum)))
        assert np.array_equal(_np(run["rv"]), once(ref.running_update(rv, want["var_unbiased"], momentum)))
        for name in ("full", "pooled"):
            if run[name] is None:
                continue
            got, exact = _np(run[name]), want[name]
            pos = exact > 0
            assert np.array_equal(got[pos], ref.to_bf16(exact[pos])), name
            assert np.all(np.abs(got - exact)[~pos] <= ref.bf16_step(exact[~pos])), name
    # routing: with beta = 8 every v is positive, dv = g_e, and with integer gradients every operation of the backward is exact
    beta8 = np.full(c, 8.0)
    for form in forms:
        run = _forward(y, gamma, beta8, rm, rv, momentum, eps, form, dtype_name)
        g_full = rng.randint(-3, 4, size=(b, h, w, c)).astype(np.float64) if form != "pooled" else None
        g_pooled = rng.randint(-3, 4, size=(b, h // 2, w // 2, c)).astype(np.float64) if form != "full" else None
        dy, dgamma, dbeta = _backward(run, form, g_full, g_pooled)
        dy_w, dgamma_w, dbeta_w, _ = ref.backward(y, gamma, beta8, eps, g_full, g_pooled)
        assert np.array_equal(_np(dbeta), dbeta_w) and np.array_equal(_np(dgamma), dgamma_w)
        assert np.array_equal(_np(dy), ref.to_bf16(dy_w)), form


def _all_outputs(y, gamma, beta, rm, rv, form, g_full, g_pooled):
    run = _forward(y, gamma, beta, rm, rv, 0.01, 1e-3, form, "float32")
    grads = _backward(run, form, g_full, g_pooled)
    return [run[k] for k in ("full", "pooled", "mean", "invstd", "rm", "rv")] + list(grads)


def test_two_calls_give_the_same_bits():
    import torch
    rng = np.random.RandomState(11)
    shape, c = (3, 37, 35), 48
    y = _random_map(shape, c, rng)
    gamma, beta, rm, rv = _params(c, rng, "float32")
    g_full, g_pooled = ref.to_bf16(rng.randn(*shape, c)), ref.to_bf16(rng.randn(3, 18, 17, c))
    first = _all_outputs(y, gamma, beta, rm, rv, "both", g_full, g_pooled)
    second = _all_outputs(y, gamma, beta, rm, rv, "both", g_full, g_pooled)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


def test_a_nan_stays_in_its_channel():
    import torch
    rng = np.random.RandomState(12)
    shape, c = (2, 7, 5), 64
    y = _random_map(shape, c, rng)
    gamma, beta, rm, rv = _params(c, rng, "float32")
    g_full, g_pooled = ref.to_bf16(rng.randn(*shape, c)), ref.to_bf16(rng.randn(2, 3, 2, c))
    clean = _all_outputs(y, gamma, beta, rm, rv, "both", g_full, g_pooled)
    bad = y.copy()
    bad[1, 3, 2, 9] = np.nan
    dirty = _all_outputs(bad, gamma, beta, rm, rv, "both", g_full, g_pooled)
    others = [k for k in range(c) if k != 9]
    for a, b in zip(clean, dirty):
        chan = (lambda t: t[:, others]) if a.dim() == 4 else (lambda t: t[others])
        only = (lambda t: t[:, 9]) if a.dim() == 4 else (lambda t: t[9])
        assert torch.equal(chan(a), chan(b))
        assert bool(torch.isnan(only(b)).all())


def test_bad_arguments_raise():
    import torch
    from ssd_keras_amd import _native as nat
    vec = lambda c: [torch.ones(c, device="cuda") for _ in range(4)]
    nhwc = lambda b, h, w, c, dt=torch.bfloat16: torch.zeros((b, h, w, c), dtype=dt, device="cuda").permute(0, 3, 1, 2)
    bad = [(nhwc(2, 4, 4, 32, torch.float32), 32),                                  # a float32 map
           (torch.zeros((2, 32, 4, 4), dtype=torch.bfloat16, device="cuda"), 32),   # NCHW memory
           (nhwc(2, 4, 4, 40), 40),                                                 # C = 40
           (nhwc(1, 1, 1, 32), 32)]                                                 # M = 1
    for y, c in bad:
        with pytest.raises(nat.SsdHipError):
            nat.bn_elu_train_forward(y, *vec(c), 0.01, 1e-3, False, True)
        mean, invstd, gamma, beta = vec(c)
        with pytest.raises(nat.SsdHipError):
            nat.bn_elu_train_backward(y, mean, invstd, gamma, beta, y, None)
