"""The convolutions of SSD7's training step against their contracts (include/ssdhip.h): ssdhip_conv_same_bias_nhwc_bf16 (forward and,
on the flipped image, data gradient; csrc/ssdhip_convbn.hip), ssdhip_ssd7_pack_filters and ssdhip_ssd7_conv_wgrad_nhwc_bf16
(csrc/ssdhip_wgrad7.hip).  Expected values are tests/np_ssd7_conv.py's float64.  Shapes are those of tests/test_conv_bn_elu_gpu.py, for
the same reasons (odd sizes that are no multiple of the 8 x 32 tile, three images, several column tiles, the notebook's width of 480
for the 5 x 5 layer), plus one 3 x 40 x 70 case per kernel size whose weight-gradient plan has at least three splits, the last shorter."""
import ctypes
import functools

import numpy as np
import pytest

from tests import np_ssd7_conv as ref

pytestmark = pytest.mark.gpu

GEOMETRIES_3 = [(32, 48), (48, 64), (64, 64), (64, 48), (48, 48), (48, 32)]
# (kernel, Cin, Cout, B, H, W)
CASES = ([(3, ci, co, 3, 19, 37) for ci, co in GEOMETRIES_3] + [(3, 32, 48, 2, 10, 150)] + [(5, 3, 32, 3, 37, 45), (5, 3, 32, 1, 6, 480)])
SPLIT_CASES = [(3, 32, 48, 3, 40, 70), (5, 3, 32, 3, 40, 70)]
WGRAD_CASES = CASES + SPLIT_CASES
ids = lambda cases: ["k%d-%dto%d-b%d-%dx%d" % c for c in cases]
BADARG = -1


def _padded_k(kernel, cin):
    return 9 * cin if kernel == 3 else 80


@functools.lru_cache(maxsize=None)
def _case(case, kind):
    """Operands (bf16-representable float64, NHWC / [Cout, k, k, Cin]) and the float64 references of one case, computed once and never
    written to: dict with x, w, bias, dy, y, dx, dw, db and, for the bounds, the same sums over absolute values (ay, adx, adw, adb)."""
    kernel, cin, cout, b, h, w = case
    rng = np.random.RandomState(hash(case) % (2 ** 31))
    if kind == "exact":
        x = rng.randint(-2, 3, size=(b, h, w, cin)).astype(np.float64)
        wt = rng.randint(-1, 2, size=(cout, kernel, kernel, cin)).astype(np.float64)
        bias = rng.randint(-8, 9, size=cout) * 0.5
        dy = rng.randint(-2, 3, size=(b, h, w, cout)).astype(np.float64)
    else:
        x, wt, bias, dy = (ref.to_bf16(rng.standard_normal(s)) for s in ((b, h, w, cin), (cout, kernel, kernel, cin), (cout,), (b, h, w, cout)))
    d = dict(x=x, w=wt, bias=bias, dy=dy, y=ref.conv_same(x, wt, bias), ay=ref.conv_same(np.abs(x), np.abs(wt)))
    d["dw"], d["db"] = ref.conv_same_weight_grad(x, dy, kernel)
    d["adw"], d["adb"] = ref.conv_same_weight_grad(np.abs(x), np.abs(dy), kernel)
    if kernel == 3:
        d["dx"], d["adx"] = ref.conv_same_input_grad(dy, wt), ref.conv_same_input_grad(np.abs(dy), np.abs(wt))
    for v in d.values():
        v.setflags(write=False)
    return d


def _map(a):
    """float64 NHWC array -> (B, C, H, W) bf16 CUDA tensor with NHWC memory."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16).cuda().permute(0, 3, 1, 2)


def _filters(wt, channels_last=True):
    """[Cout, k, k, Cin] float64 -> (Cout, Cin, k, k) bf16 CUDA tensor in either memory order."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(wt)).to(torch.bfloat16).cuda().permute(0, 3, 1, 2)
    return t if channels_last else t.contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).double().cpu().numpy()


def _bits(t):
    import torch
    return t.contiguous().view(torch.int16).cpu().numpy()


def _bf16_bits_of(a):
    import torch
    return _bits(torch.from_numpy(np.ascontiguousarray(a)).to(torch.bfloat16))


def _forward(case, kind):
    from ssd_keras_amd import _native as nat
    import torch
    d = _case(case, kind)
    packed = nat.conv_bn_elu_pack(_filters(d["w"]))
    y = nat.ssd7_conv_bias(_map(d["x"]), packed, torch.from_numpy(d["bias"]).to(torch.bfloat16).cuda(), case[2], case[0])
    torch.cuda.synchronize()
    return y


def _dgrad(case, kind):
    from ssd_keras_amd import _native as nat
    import torch
    d = _case(case, kind)
    packed = nat.conv_bn_elu_pack(_filters(d["w"]).flip(2, 3).transpose(0, 1))
    dx = nat.ssd7_conv_bias(_map(d["dy"]), packed, None, case[1], 3)
    torch.cuda.synchronize()
    return dx


def _wgrad(case, kind, like=None):
    from ssd_keras_amd import _native as nat
    import torch
    d = _case(case, kind)
    dw, db = nat.ssd7_conv_wgrad(_map(d["x"]), _map(d["dy"]), case[0], like=like)
    torch.cuda.synchronize()
    return dw, db


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_exact_arithmetic_forward_and_data_gradient(case):
    """x in -2 .. 2, w in {-1, 0, 1}, bias a multiple of 0.5: |acc| <= 2 * 576 and acc + bias is exact in float32, so the result must be
    the rounding of the exact value bit for bit, everywhere; the data gradient through the flipped image likewise."""
    d = _case(case, "exact")
    assert np.abs(d["y"]).max() < 2 ** 24 and np.array_equal(d["y"], d["y"].astype(np.float32))
    y = _forward(case, "exact")
    assert y.permute(0, 2, 3, 1).is_contiguous() and tuple(y.shape) == (case[3], case[2], case[4], case[5])
    assert np.array_equal(_bits(y.permute(0, 2, 3, 1)), _bf16_bits_of(d["y"]))
    if case[0] == 3:
        dx = _dgrad(case, "exact")
        assert tuple(dx.shape) == (case[3], case[1], case[4], case[5])
        assert np.array_equal(_bits(dx.permute(0, 2, 3, 1)), _bf16_bits_of(d["dx"]))


def _like(case, dtype, channels_last):
    import torch
    k, cin, cout = case[:3]
    t = torch.empty((cout, cin, k, k), dtype=dtype, device="cuda")
    return t.contiguous(memory_format=torch.channels_last) if channels_last else t


@pytest.mark.parametrize("case", WGRAD_CASES, ids=ids(WGRAD_CASES))
def test_exact_arithmetic_weight_and_bias_gradient(case):
    """x, dy in -2 .. 2: every partial and total is an integer of at most 4 * 8400 < 2^24 -- float32 output must equal the exact
    integers bit for bit (dense default and both memory orders of `like`), bf16 output their one rounding."""
    import torch
    from ssd_keras_amd import _native as nat
    d = _case(case, "exact")
    assert np.abs(d["adw"]).max() <= 4 * 8400
    if case in SPLIT_CASES:
        splits, per, tiles, last = nat.ssd7_conv_wgrad_plan(case[3], case[4], case[5], case[1], case[2], case[0])
        print("plan of %s: %d splits of %d tiles, the last %d (of %d)" % (case, splits, per, last, tiles))
        assert splits >= 3 and last < per
    want_dw, want_db = d["dw"].transpose(0, 3, 1, 2), d["db"]
    dw, db = _wgrad(case, "exact")
    assert dw.dtype == torch.float32 and dw.permute(0, 2, 3, 1).is_contiguous()
    assert np.array_equal(dw.double().cpu().numpy(), want_dw) and np.array_equal(db.double().cpu().numpy(), want_db)
    for channels_last in (False, True):
        like = _like(case, torch.float32, channels_last)
        dw, db = _wgrad(case, "exact", like)
        assert dw.stride() == like.stride() and np.array_equal(dw.double().cpu().numpy(), want_dw)
        assert np.array_equal(db.double().cpu().numpy(), want_db)
        like = _like(case, torch.bfloat16, channels_last)
        dw, db = _wgrad(case, "exact", like)
        assert dw.dtype == torch.bfloat16 and dw.stride() == like.stride()
        assert np.array_equal(_bits(dw), _bf16_bits_of(want_dw)) and np.array_equal(_bits(db), _bf16_bits_of(want_db))


def _excess(got, want, k_len, mag, rounded=True):
    """error - bound per element: 2^-8 |want| (the bf16 rounding, where there is one) + K 2^-24 sum |a||b| (a length-K float32 sum)."""
    return np.abs(got - want) - ((2.0 ** -8 * np.abs(want) if rounded else 0.0) + k_len * 2.0 ** -24 * mag)


@pytest.mark.parametrize("case", CASES, ids=ids(CASES))
def test_random_values_forward_and_data_gradient(case):
    """N(0, 1) operands rounded to bf16.  K: the padded contraction length, 9 Cin (data gradient: 9 Cout) or 80; the magnitude is
    sum |x||w|.  bf16 products are exact in float32, so K terms cost at most K - 1 roundings: the K-th covers the accumulator's share of
    the bias add's rounding, and the bias's own share (2^-24 |bias| at most) lies inside the 2^-8 |want| term, of which the final
    rounding needs half."""
    d = _case(case, "random")
    e = _excess(_nhwc(_forward(case, "random")), d["y"], _padded_k(case[0], case[1]), d["ay"])
    print("random %s forward: largest (error - bound) %.3g" % (case, e.max()))
    assert e.max() <= 0
    if case[0] == 3:
        e = _excess(_nhwc(_dgrad(case, "random")), d["dx"], 9 * case[2], d["adx"])
        print("random %s data gradient: largest (error - bound) %.3g" % (case, e.max()))
        assert e.max() <= 0


@pytest.mark.parametrize("case", WGRAD_CASES, ids=ids(WGRAD_CASES))
def test_random_values_weight_and_bias_gradient(case):
    """K: the padded positions, 256 per 8 x 32 tile.  float32 output carries no rounding term, bf16 output one."""
    import torch
    d = _case(case, "random")
    k, cin, cout, b, h, w = case
    k_len = b * -(-h // 8) * -(-w // 32) * 256
    want_dw = d["dw"].transpose(0, 3, 1, 2)
    for dtype in (torch.float32, torch.bfloat16):
        dw, db = _wgrad(case, "random", _like(case, dtype, True))
        rounded = dtype == torch.bfloat16
        e_w = _excess(dw.double().cpu().numpy(), want_dw, k_len, d["adw"].transpose(0, 3, 1, 2), rounded)
        e_b = _excess(db.double().cpu().numpy(), d["db"], k_len, d["adb"], rounded)
        print("random %s weight gradient (%s): largest (error - bound) dw %.3g db %.3g" % (case, dtype, e_w.max(), e_b.max()))
        assert e_w.max() <= 0 and e_b.max() <= 0


@pytest.mark.parametrize("channels_last", [False, True], ids=["contiguous", "channels_last"])
def test_pack_launch_writes_every_byte_of_all_seven_layers(channels_last):
    """Buffers prefilled with 0xFF bytes; one launch for the seven layers: the forward image equals conv_bn_elu_pack(w), the flipped one
    conv_bn_elu_pack(w.flip(2, 3).transpose(0, 1)), byte for byte."""
    import torch
    from ssd_keras_amd import _native as nat
    rng = np.random.RandomState(5)
    weights = [_filters(rng.standard_normal((cout, k, k, cin)), channels_last) for k, cin, cout in ref.LAYERS]
    assert all(wt.is_contiguous() != channels_last or wt.shape[1] == 1 for wt in weights)
    fwd, flipped = nat.ssd7_pack_images(weights)
    assert flipped[0] is None and all(t is not None for t in flipped[1:])
    for t in fwd + flipped[1:]:
        t.view(torch.uint8).fill_(0xFF)
    nat.ssd7_pack_filters(weights, fwd, flipped)
    torch.cuda.synchronize()
    for wt, f, t in zip(weights, fwd, flipped):
        assert np.array_equal(_bits(f), _bits(nat.conv_bn_elu_pack(wt).reshape(-1)))
        if t is not None:
            assert np.array_equal(_bits(t), _bits(nat.conv_bn_elu_pack(wt.flip(2, 3).transpose(0, 1)).reshape(-1)))


@pytest.mark.parametrize("case", [CASES[4], CASES[5], CASES[1], CASES[7]], ids=ids([CASES[4], CASES[5], CASES[1], CASES[7]]))
def test_no_cross_talk(case):
    """A NaN in one input channel of x reaches only dw[..., ci]; a NaN in one channel of dy only dw[co] and db[co].  The 48-channel
    layers run as two 32-channel blocks whose last 16 lanes read past the pixel's values, the 5 x 5 layer's kernel row has a sixteenth
    column: what those lanes see must stay out of every sum (nothing else is NaN, and the exact tests leave no room for a finite leak)."""
    import torch
    from ssd_keras_amd import _native as nat
    d = _case(case, "exact")
    k, cin, cout = case[:3]
    ci, co = cin - 1, cout // 2
    x, dy = d["x"].copy(), d["dy"].copy()
    x[1, 3, 5, ci] = np.nan
    dw, db = nat.ssd7_conv_wgrad(_map(x), _map(d["dy"]), k)
    nan = np.isnan(dw.double().cpu().numpy())                     # (Cout, Cin, k, k)
    assert nan[:, ci].any() and not np.delete(nan, ci, axis=1).any() and not bool(torch.isnan(db).any())
    assert np.array_equal(np.delete(dw.double().cpu().numpy(), ci, axis=1), np.delete(d["dw"].transpose(0, 3, 1, 2), ci, axis=1))
    dy[2, 4, 6, co] = np.nan
    dw, db = nat.ssd7_conv_wgrad(_map(d["x"]), _map(dy), k)
    nan, nan_b = np.isnan(dw.double().cpu().numpy()), np.isnan(db.double().cpu().numpy())
    assert nan[co].all() and not np.delete(nan, co, axis=0).any()
    assert nan_b[co] and not np.delete(nan_b, co).any()
    # forward: a NaN input channel poisons the 5 x 5 window around its pixel for every output channel and nothing else
    packed = nat.conv_bn_elu_pack(_filters(np.ones_like(d["w"])))
    y = nat.ssd7_conv_bias(_map(x), packed, None, cout, k)
    want = np.zeros(d["y"].shape[:3], dtype=bool)
    r = k // 2
    want[1, 3 - r:3 + r + 1, 5 - r:5 + r + 1] = True
    assert np.array_equal(np.isnan(_nhwc(y)), np.broadcast_to(want[..., None], d["y"].shape))


@pytest.mark.parametrize("case", [CASES[2], SPLIT_CASES[0], SPLIT_CASES[1]], ids=ids([CASES[2], SPLIT_CASES[0], SPLIT_CASES[1]]))
def test_two_calls_are_bit_equal(case):
    import torch
    a, b = _wgrad(case, "random"), _wgrad(case, "random")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(_forward(case, "random"), _forward(case, "random"))


def test_pack_launch_refusals():
    """ssdhip_ssd7_pack_filters: more than eight layers, none, a flipped image for the 5 x 5 layer, a geometry SSD7 does not have, a
    negative stride, an odd pointer and a missing array are SSDHIP_E_BADARG; nothing is launched, the images stay as they were."""
    import torch
    from ssd_keras_amd import _native as nat
    lib = nat.load()
    w3 = torch.zeros((48, 32, 3, 3), dtype=torch.bfloat16, device="cuda")
    w5 = torch.zeros((32, 3, 5, 5), dtype=torch.bfloat16, device="cuda")
    (f3, f5), (t3, _) = nat.ssd7_pack_images([w3, w5])
    for t in (f3, f5, t3):
        t.fill_(7.0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(weights, fwd, flipped, cin, cout, kernel, strides, n=None):
        n = len(weights) if n is None else n
        ptrs = lambda ts: (ctypes.c_void_p * max(len(ts), 1))(*ts)
        ints = lambda vs: (ctypes.c_int * max(len(vs), 1))(*vs)
        return lib.ssdhip_ssd7_pack_filters(n, ptrs(weights), ptrs(fwd), ptrs(flipped), ints(cin), ints(cout), ints(kernel),
                                            (ctypes.c_longlong * max(len(strides), 1))(*strides), stream)

    p = lambda t, off=0: t.data_ptr() + off
    s3, s5 = list(w3.stride()), list(w5.stride())
    good = ([p(w3)], [p(f3)], [p(t3)], [32], [48], [3], s3)
    assert call(*[v * 9 for v in good]) == BADARG and call(*good, n=0) == BADARG                     # nine layers; none
    assert call([p(w5)], [p(f5)], [p(t3)], [3], [32], [5], s5) == BADARG                                 # a flipped image for k = 5
    assert call([p(w3)], [p(f3)], [p(t3)], [40], [48], [3], s3) == BADARG                                # not one of SSD7's layers
    assert call([p(w3)], [p(f3)], [p(t3)], [32], [48], [3], s3[:2] + [-1, 1]) == BADARG                  # negative stride
    assert call([p(w3, 1)], [p(f3)], [p(t3)], [32], [48], [3], s3) == BADARG                             # odd pointers
    assert call([p(w3)], [p(f3, 1)], [p(t3)], [32], [48], [3], s3) == BADARG
    assert call([p(w3)], [None], [p(t3)], [32], [48], [3], s3) == BADARG                                 # no forward image
    assert lib.ssdhip_ssd7_pack_filters(1, None, None, None, None, None, None, None, stream) == BADARG
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (f3, f5, t3))
    with pytest.raises(nat.SsdHipError):
        nat.ssd7_pack_filters([w3], [f5], [t3])
    with pytest.raises(nat.SsdHipError):
        nat.ssd7_pack_filters([w3.float()], [f3], [t3])
    assert call(*good) == 0                                                                              # and the good call is accepted


def test_refusals_launch_nothing():
    """The refused geometries of test_conv_bn_elu_gpu.py's test_unsupported_geometry_is_refused, a misaligned pointer and a workspace
    that is too small: SSDHIP_E_BADARG, the outputs untouched."""
    import torch
    from ssd_keras_amd import _native as nat
    lib = nat.load()
    x = torch.zeros((1, 8, 8, 64), dtype=torch.bfloat16, device="cuda")
    dy = torch.ones((1, 8, 8, 64), dtype=torch.bfloat16, device="cuda")
    w = torch.zeros((9 * 64 * 72,), dtype=torch.bfloat16, device="cuda")
    y = torch.full((1, 8, 8, 64), 7.0, dtype=torch.bfloat16, device="cuda")
    dw = torch.full((64 * 9 * 64,), 7.0, dtype=torch.float32, device="cuda")
    db = torch.full((64,), 7.0, dtype=torch.float32, device="cuda")
    ws = torch.full((1 << 20,), 7.0, dtype=torch.float32, device="cuda")
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    conv = lambda xp, wp, yp, cin, cout, k: lib.ssdhip_conv_same_bias_nhwc_bf16(xp, wp, None, yp, 1, 8, 8, cin, cout, k, stream)
    wgrad = lambda xp, dyp, dwp, wsp, nbytes, cin, cout, k: lib.ssdhip_ssd7_conv_wgrad_nhwc_bf16(
        xp, dyp, dwp, p(db), 1, 8, 8, cin, cout, k, 0, None, wsp, nbytes, stream)
    for cin, cout, k in ((40, 48, 3), (32, 40, 3), (3, 32, 3), (32, 48, 5)):
        assert conv(p(x), p(w), p(y), cin, cout, k) == BADARG
        assert wgrad(p(x), p(dy), p(dw), p(ws), ws.numel() * 4, cin, cout, k) == BADARG
        assert lib.ssdhip_ssd7_conv_wgrad_workspace_bytes(1, 8, 8, cin, cout, k) == 0
    need = lib.ssdhip_ssd7_conv_wgrad_workspace_bytes(1, 8, 8, 64, 64, 3)
    assert need == (64 * 9 * 64 + 64) * 4 * nat.ssd7_conv_wgrad_plan(1, 8, 8, 64, 64, 3)[0]
    assert conv(p(x, 2), p(w), p(y), 64, 64, 3) == BADARG and conv(p(x), p(w, 2), p(y), 64, 64, 3) == BADARG
    assert conv(p(x), p(w), p(y, 2), 64, 64, 3) == BADARG and conv(None, p(w), p(y), 64, 64, 3) == BADARG
    assert wgrad(p(x, 2), p(dy), p(dw), p(ws), need, 64, 64, 3) == BADARG and wgrad(p(x), p(dy, 2), p(dw), p(ws), need, 64, 64, 3) == BADARG
    assert wgrad(p(x), p(dy), p(dw, 2), p(ws), need, 64, 64, 3) == BADARG and wgrad(p(x), p(dy), p(dw), p(ws, 4), need, 64, 64, 3) == BADARG
    assert wgrad(p(x), p(dy), p(dw), p(ws), need - 1, 64, 64, 3) == BADARG
    bad = (ctypes.c_longlong * 4)(1, 1, -1, 1)
    assert lib.ssdhip_ssd7_conv_wgrad_nhwc_bf16(p(x), p(dy), p(dw), p(db), 1, 8, 8, 64, 64, 3, 0, bad, p(ws), need, stream) == BADARG
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (y, dw, db, ws))
    with pytest.raises(nat.SsdHipError):
        nat.ssd7_conv_wgrad(x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)[:, :40], 3)
    with pytest.raises(nat.SsdHipError):
        nat.ssd7_conv_bias(x.permute(0, 3, 1, 2), w[:100], None, 64, 3)
