"""csrc/ssdhip_convbn.hip against its numerical contract (include/ssdhip.h, ssdhip_conv_bn_elu_nhwc_bf16):

    v = fmaf(acc, scale[c], shift[c]);  e = v > 0 ? v : expm1f(v);  [maximum of the 2 x 2 window's four e;]  one rounding to bf16

for every geometry of SSD7 (reference models/keras_ssd7.py:277-309), with and without the fused 'valid' pool.  The expected values are
float64 NumPy / torch on the CPU: convolution, v, ELU through expm1, maximum, one rounding.  Shapes are the smallest that reach every
edge: odd heights and widths that are no multiple of the 8 x 32 tile, three images (the padding between images), several column tiles,
an even and an odd height and the notebook's width of 480 for the 5 x 5 layer."""
import ctypes
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GEOMETRIES_3 = [(32, 48), (48, 64), (64, 64), (64, 48), (48, 48), (48, 32)]
# (kernel, Cin, Cout, B, H, W)
CASES = ([(3, ci, co, 3, 19, 37) for ci, co in GEOMETRIES_3] + [(3, 32, 48, 2, 10, 150)] +
         [(5, 3, 32, 3, 37, 45), (5, 3, 32, 3, 38, 45), (5, 3, 32, 1, 6, 480)])
IDS = ["k%d-%dto%d-b%d-%dx%d" % c for c in CASES]


def _padded_k(kernel, cin):
    return 9 * cin if kernel == 3 else 80


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    """Operands (already bf16-representable float64 / float32 tables) and the float64 reference of one case, computed once:
    (x [B, Cin, H, W], w [Cout, Cin, k, k], scale, shift, e [B, Cout, H, W] = elu(conv * scale + shift), err2 [B, Cout, H, W] =
    K 2^-24 |scale_c| conv(|x|, |w|): the bound of a length-K float32 sum, scaled like the sum)."""
    import torch
    import torch.nn.functional as F
    kernel, cin, cout, b, h, w = case
    rng = np.random.RandomState(hash(case) % (2 ** 31))
    if kind == "exact":
        x = rng.randint(-2, 3, size=(b, cin, h, w)).astype(np.float64)
        wt = rng.randint(-1, 2, size=(cout, cin, kernel, kernel)).astype(np.float64)
        scale = rng.choice([-0.5, 0.5, 1.0, 2.0], size=cout).astype(np.float32)
        shift = (rng.randint(-8, 9, size=cout) * 0.5).astype(np.float32)
    else:
        bf = lambda a: torch.from_numpy(a).to(torch.bfloat16).double().numpy()
        x = bf(rng.standard_normal((b, cin, h, w)).astype(np.float32))
        wt = bf(rng.standard_normal((cout, cin, kernel, kernel)).astype(np.float32))
        gamma = rng.uniform(0.5, 1.5, size=cout) * rng.choice([-1.0, 1.0], size=cout)
        var, mean, beta, bias = rng.uniform(0.1, 4.0, size=cout), rng.standard_normal(cout), rng.standard_normal(cout), rng.standard_normal(cout)
        s64 = gamma / np.sqrt(var + 1e-3)
        scale, shift = s64.astype(np.float32), (beta + (bias - mean) * s64).astype(np.float32)
    xt, wtt = torch.from_numpy(x), torch.from_numpy(wt)
    acc = F.conv2d(xt, wtt, padding=kernel // 2).numpy()
    mag = F.conv2d(xt.abs(), wtt.abs(), padding=kernel // 2).numpy()
    s, t = scale.astype(np.float64).reshape(1, -1, 1, 1), shift.astype(np.float64).reshape(1, -1, 1, 1)
    v = acc * s + t
    e = np.where(v > 0, v, np.expm1(np.minimum(v, 0)))
    err2 = _padded_k(kernel, cin) * 2.0 ** -24 * np.abs(s) * mag
    if kind == "exact":
        assert np.abs(acc).max() < 2 ** 11 and np.array_equal(v, v.astype(np.float32))
    return x, wt, scale, shift, e, err2


def _pool(a):
    """MaxPooling2D(2, 2) 'valid' of (B, C, H, W): the last row / column of an odd map feeds nothing."""
    b, c, h, w = a.shape
    a = a[:, :, :h // 2 * 2, :w // 2 * 2].reshape(b, c, h // 2, 2, w // 2, 2)
    return a.max(axis=(3, 5))


def _run(case, kind, pool):
    import torch
    from ssd_keras_amd import _native as nat
    x, wt, scale, shift, _, _ = _case(case, kind)
    xg = torch.from_numpy(x).to(torch.bfloat16).cuda().contiguous(memory_format=torch.channels_last)
    packed = nat.conv_bn_elu_pack(torch.from_numpy(wt).cuda())
    y = nat.conv_bn_elu(xg, packed, torch.from_numpy(scale).cuda(), torch.from_numpy(shift).cuda(), case[0], pool)
    torch.cuda.synchronize()
    assert y.dtype == torch.bfloat16 and y.permute(0, 2, 3, 1).is_contiguous()
    return y


def _ordered(t):
    """bf16 tensor -> integers whose difference counts bf16 steps (both zeros are 0)."""
    import torch
    bits = t.contiguous().view(torch.int16).cpu().numpy().astype(np.int64) & 0xffff
    return np.where(bits < 0x8000, bits, -(bits & 0x7fff))


@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_exact_arithmetic(case, pool):
    """Small integers: every accumulator is an integer below 2^11 and v is exact in float32, so the summation order cannot matter.
    Where the expected value is positive the result must equal its rounding bit for bit; elsewhere one bf16 step is allowed (expm1f
    against expm1)."""
    import torch
    e = _case(case, "exact")[4]
    want = _pool(e) if pool else e
    got = _run(case, "exact", pool)
    assert tuple(got.shape) == want.shape
    want_bf = torch.from_numpy(want).to(torch.bfloat16)
    g, w = _ordered(got), _ordered(want_bf)
    pos = want > 0
    print("exact %s pool=%d: %d positive values, %d differ; others: max %d steps" % (
        case, pool, pos.sum(), (g[pos] != w[pos]).sum(), np.abs(g[~pos] - w[~pos]).max() if (~pos).any() else 0))
    assert np.array_equal(g[pos], w[pos])
    assert np.abs(g[~pos] - w[~pos]).max() <= 1


@pytest.mark.parametrize("pool", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_random_values(case, pool):
    """N(0, 1) operands rounded to bf16, gamma of both signs, running_var in [0.1, 4].  Bound per element:
    2^-8 |want| (one bf16 step: the final rounding and a double rounding) + K 2^-24 |scale_c| A (the standard bound on a length-K
    float32 sum; A = conv(|x|, |w|) at the element, K the padded K).  ELU is 1-Lipschitz and a maximum moves by at most the largest
    move of its arguments, so a pooled element takes the largest second term of its window."""
    _, _, _, _, e, err2 = _case(case, "random")
    want, err2 = (_pool(e), _pool(err2)) if pool else (e, err2)
    got = _run(case, "random", pool).double().cpu().numpy()
    assert got.shape == want.shape
    excess = np.abs(got - want) - (2.0 ** -8 * np.abs(want) + err2)
    print("random %s pool=%d: largest |got - want| %.3g, largest (error - bound) %.3g" % (case, pool, np.abs(got - want).max(), excess.max()))
    assert excess.max() <= 0


@pytest.mark.parametrize("case", [CASES[0], CASES[6], CASES[7], CASES[8]], ids=[IDS[0], IDS[6], IDS[7], IDS[8]])
def test_pool_equals_unpooled_then_max(case):
    """Rounding is monotonic: the fused pool equals the unpooled launch followed by a 2 x 2 'valid' maximum of the bf16 map."""
    import torch
    import torch.nn.functional as F
    full, pooled = _run(case, "random", 0), _run(case, "random", 1)
    assert torch.equal(pooled.float(), F.max_pool2d(full.float(), 2, 2))


def test_unsupported_geometry_is_refused():
    """Cin = 40 (and every other geometry SSD7 does not have): the bad-argument code, no launch, the output untouched."""
    import torch
    from ssd_keras_amd import _native as nat
    lib = nat.load()
    assert lib.ssdhip_conv_bn_elu_pack_bytes(40, 48, 3) == 0 and lib.ssdhip_conv_bn_elu_pack_bytes(3, 32, 3) == 0
    # [3 x 3 taps][48 -> 64 filter rows][32 + 8 values] and [5 kernel rows][32][16] bf16
    assert lib.ssdhip_conv_bn_elu_pack_bytes(32, 48, 3) == 9 * 64 * (32 + 8) * 2 and lib.ssdhip_conv_bn_elu_pack_bytes(3, 32, 5) == 5 * 32 * 16 * 2
    x = torch.zeros((1, 8, 8, 40), dtype=torch.bfloat16, device="cuda")
    w = torch.zeros((9 * 64 * 48,), dtype=torch.bfloat16, device="cuda")
    tab = torch.ones((48,), dtype=torch.float32, device="cuda")
    y = torch.full((1, 8, 8, 48), 7.0, dtype=torch.bfloat16, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for cin, cout, k in ((40, 48, 3), (32, 40, 3), (3, 32, 3), (32, 48, 5)):
        assert lib.ssdhip_conv_bn_elu_nhwc_bf16(p(x), p(w), p(tab), p(tab), p(y), 1, 8, 8, cin, cout, k, 0, stream) == -1     # SSDHIP_E_BADARG
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    with pytest.raises(nat.SsdHipError):
        nat.conv_bn_elu_pack(torch.zeros((48, 40, 3, 3), device="cuda"))
    with pytest.raises(nat.SsdHipError):
        nat.conv_bn_elu(x.permute(0, 3, 1, 2), w, tab, tab, 3, False)
