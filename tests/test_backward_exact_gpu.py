"""The backward kernels of the VGG / SSD300 training step against tests/np_conv_grads.py (float64) on data where float32 accumulation is
exact in any order (tests/backward_exact_cases.py): every comparison is bit equality -- the float64 result as it is for float32
outputs, rounded once (`to_bf16`) for bf16 outputs -- so one dropped, doubled or misplaced term of a sum over positions, K slices or
tiles shows.  Covered: the three weight-gradient kernels of csrc/ssdhip_wgrad.hip with the bias partials in their reduction launch,
the ReLU-mask / channel-sum passes, embed_strided and conv1_1_bwd_kernel of csrc/ssdhip_train.hip, and the data gradients through
the forward kernels on flipped, transposed filters (implicit GEMM, resident-filter Cin = 64, image-resident, slab with the ReLU mask
and the bias partial sums of its epilogue).  Each case asserts, from the library's plan exports, that it reaches the seam its
comment in the case table names.  Needs an MI355X."""
import functools

import numpy as np
import pytest

from tests import backward_exact_cases as cases
from tests import np_conv_grads as ref

pytestmark = pytest.mark.gpu


def _nat():
    from ssd_keras_amd import _native as nat
    return nat


def _nhwc(a):
    """[N, H, W, C] float64 array of bf16 values -> (N, C, H, W) bf16 CUDA tensor with NHWC memory (a map, or [Cout, k, k, Cin] filters)."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.bfloat16).cuda().permute(0, 3, 1, 2)


def _np(t):
    """A device tensor as float64, 4-D ones in their NHWC / [Cout, k, k, Cin] order."""
    t = t.detach().double().cpu()
    return (t.permute(0, 2, 3, 1) if t.dim() == 4 else t).numpy()


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = got != want
    n = int(diff.sum())
    if n:
        first = tuple(int(i) for i in np.argwhere(diff)[0])
        msg = "%s: %d of %d elements differ, the first at %s: got %r, want %r" % (what, n, diff.size, first, got[first], want[first])
        print(msg)
        raise AssertionError(msg)
    assert np.array_equal(got, want)


def _weight_gradient(call, x, dy, want, what):
    """One weight-gradient call with the bias partials of dy riding in its reduction launch: dw and db are the exact integer sums."""
    nat = _nat()
    xd, dyd = _nhwc(x), _nhwc(dy)
    out = call(xd, dyd, nat.channel_sums_partial(dyd))
    assert out is not None, "geometry must be supported"
    gw, gb = out
    import torch
    assert gw.dtype == torch.float32 and gb.dtype == torch.float32
    _same(_np(gw), want, what + " dw")
    _same(_np(gb), ref.channel_sums(dy), what + " db")


@pytest.mark.parametrize("case,plan", cases.WG1_CASES)
def test_1x1_weight_gradient(case, plan):
    nat = _nat()
    cases.check_wg1_plan(case, plan)
    b, h, w, cin, cout = case
    x, dy = cases.wgrad_data(case, (b, h, w, cin), (b, h, w, cout))
    _weight_gradient(lambda xd, dyd, part: nat.conv1x1_wgrad(xd, dyd, bias_partial=part), x, dy, ref.conv_weight_grad(x, dy, 1, 0, 1, 1),
                     "conv1x1_wgrad %s" % (case,))


@pytest.mark.parametrize("case,plan", cases.TAP_CASES)
def test_tap_gathered_weight_gradient(case, plan):
    nat = _nat()
    cases.check_tap_plan(case, plan)
    b, h, w, cin, cout, s, p, d = case
    x, dy = cases.wgrad_data(case, (b, h, w, cin), cases.tap_out_shape(case))
    _weight_gradient(lambda xd, dyd, part: nat.conv3x3_taps_wgrad(xd, dyd, s, p, d, bias_partial=part), x, dy,
                     ref.conv_weight_grad(x, dy, s, p, d, 3), "conv3x3_taps_wgrad %s" % (case,))


@pytest.mark.parametrize("case,plan", cases.GRID_CASES)
def test_position_grid_weight_gradient(case, plan):
    nat = _nat()
    cases.check_grid_plan(case, plan)
    b, h, w, cin, cout = case
    x, dy = cases.wgrad_data(case, (b, h, w, cin), (b, h, w, cout))
    _weight_gradient(lambda xd, dyd, part: nat.conv3x3_wgrad(xd, dyd, bias_partial=part), x, dy, ref.conv_weight_grad(x, dy, 1, 1, 1, 3),
                     "conv3x3_wgrad %s" % (case,))


@functools.lru_cache(maxsize=None)
def _dilated(case):
    b, h, w, cin, cout = case
    x, dy = cases.wgrad_data(case, (b, h, w, cin), (b, h, w, cout))
    return x, dy, ref.conv_weight_grad(x, dy, 1, 6, 6, 3)


@pytest.mark.parametrize("gather", [False, True])
@pytest.mark.parametrize("case,plan", cases.DILATED_CASES)
def test_dilated_weight_gradient_on_the_grid_and_with_gathered_taps(case, plan, gather, monkeypatch):
    nat = _nat()
    cases.check_dilated_plan(case, plan)
    if gather:
        monkeypatch.setenv("SSDHIP_WGRAD_GATHER_ONLY", "1")
    x, dy, want = _dilated(case)
    _weight_gradient(lambda xd, dyd, part: nat.conv3x3_taps_wgrad(xd, dyd, 1, 6, 6, bias_partial=part), x, dy, want,
                     "conv3x3_taps_wgrad dilation 6 %s%s" % (case, " gathered" if gather else ""))


@pytest.mark.parametrize("case,plan", cases.MASK_CASES)
def test_relu_mask_and_channel_sums(case, plan):
    nat = _nat()
    cases.check_mask_plan(case, plan)
    _, gy = cases.wgrad_data(case, (1, 1, 1, 8), case)
    act = cases.activation(case, case)
    want = ref.relu_mask(gy, act)
    gyd, actd = _nhwc(gy), _nhwc(act)
    out, partial = nat.relu_bwd_bias(gyd, actd, reduce=False)
    assert partial.shape == (plan[0], case[3])
    _same(_np(out), want, "relu_bwd_bias map")
    _same(_np(partial).sum(axis=0), ref.channel_sums(want), "relu_bwd_bias partial rows")
    _same(_np(nat.relu_bwd_bias(gyd, actd)[1]), ref.channel_sums(want), "relu_bwd_bias sums")
    _same(_np(nat.channel_sums_partial(gyd)).sum(axis=0), ref.channel_sums(gy), "channel_sums_partial rows")


def _filters(w):
    """[Cout, k, k, Cin] filters -> the device tensor a forward kernel takes to compute the layer's data gradient."""
    return _nhwc(cases.flipped(w))


def _masked_with_sums(gyd, wtd, act, want, what):
    """conv3x3_halo_masked with its epilogue's sums: the masked map is exact, and the partial rows add up -- in float64, exactly -- to the
    channel sums of that map."""
    nat = _nat()
    got, part = nat.conv3x3_halo_masked(gyd, wtd, _nhwc(act), sums=True)
    masked = ref.to_bf16(ref.relu_mask(want, act))
    _same(_np(got), masked, what + " masked map")
    _same(_np(part).sum(axis=0), ref.channel_sums(_np(got)), what + " partial rows against its own output")
    return got, part, masked


@pytest.mark.parametrize("case,plan", cases.SLAB_CASES)
def test_data_gradient_through_the_slab_kernel(case, plan):
    nat = _nat()
    cases.check_slab_plan(case, plan)
    b, h, w, cy, cx = case
    gy, wt = cases.dgrad_data(case, (b, h, w, cy), (cy, 3, 3, cx))
    want = ref.conv_input_grad(gy, wt, (b, h, w, cx), 1, 1, 1)
    share = cases.share_within_256(want)
    print("%s: %.4f of the outputs within +-256" % (case, share))
    assert share >= 0.99
    gyd, wtd = _nhwc(gy), _filters(wt)
    _same(_np(nat.conv2d_same(gyd, wtd, None, relu=False)), ref.to_bf16(want), "conv2d_same %s" % (case,))
    if nat.conv3x3_image_supported(gyd, wtd, 1):
        _same(_np(nat.conv3x3_image(gyd, wtd, None, relu=False)), ref.to_bf16(want), "conv3x3_image %s" % (case,))
    _masked_with_sums(gyd, wtd, cases.activation(case, (b, h, w, cx)), want, "conv3x3_halo_masked %s" % (case,))


@pytest.mark.parametrize("case", cases.FORWARD_CASES)
def test_data_gradient_through_the_other_forward_kernels(case):
    nat = _nat()
    b, h, w, cy, cx, k, d, kernels = case
    gy, wt = cases.dgrad_data(case, (b, h, w, cy), (cy, k, k, cx))
    want = ref.to_bf16(ref.conv_input_grad(gy, wt, (b, h, w, cx), 1, d * (k // 2), d))
    gyd, wtd = _nhwc(gy), _filters(wt)
    run = {"same": lambda: nat.conv2d_same(gyd, wtd, None, dilation=d, relu=False),
           "c64": lambda: nat.conv3x3_c64(gyd, wtd, None, relu=False, pool=False),
           "image": lambda: nat.conv3x3_image(gyd, wtd, None, dilation=d, relu=False)}
    assert "image" not in kernels or nat.conv3x3_image_supported(gyd, wtd, d)
    for name in kernels:
        _same(_np(run[name]()), want, "%s %s" % (name, case[:7]))


@pytest.mark.parametrize("case", cases.STRIDED_CASES)
def test_strided_and_valid_layers(case):
    nat = _nat()
    from ssd_keras_amd.models import _common as cm
    b, h, w, cin, cout, s, p = case
    ho, wo = ref.out_size(h, s, p, 1, 3), ref.out_size(w, s, p, 1, 3)
    x, dy = cases.wgrad_data(case, (b, h, w, cin), (b, ho, wo, cout))
    _, wt = cases.dgrad_data(case, (1, 1, 1, 1), (cout, 3, 3, cin))
    xd, dyd, wd = _nhwc(x), _nhwc(dy), _nhwc(wt)
    _same(_np(nat.embed_strided(dyd, h, w, s, 1 - p)), ref.embed_strided(dy, h, w, s, 1 - p), "embed_strided %s" % (case,))
    gx, gw, gb = cm._conv_input_weight_grads(dyd, xd, wd, (s, s), (p, p), (1, 1), True, None, nat.channel_sums_partial(dyd))
    assert gb is not None
    _same(_np(gx), ref.to_bf16(ref.conv_input_grad(dy, wt, (b, h, w, cin), s, p, 1)), "gx %s" % (case,))
    _same(_np(gw), ref.conv_weight_grad(x, dy, s, p, 1, 3), "gw %s" % (case,))
    _same(_np(gb), ref.channel_sums(dy), "gb %s" % (case,))


@pytest.mark.parametrize("case,blocks", cases.FIRST_LAYER_CASES)
def test_first_layer_backward(case, blocks):
    nat = _nat()
    cases.check_first_layer_plan(case, blocks)
    b, h, w = case
    _, gy = cases.wgrad_data(case, (1, 1, 1, 8), (b, h, w, 64))
    act = cases.activation(case, (b, h, w, 64))
    x = cases.ints(np.random.RandomState(b * h * w), (b, h, w, 3), [-3, -2, -1, 0, 1, 2, 3])
    gw, gb = nat.conv1_1_backward(_nhwc(gy), _nhwc(act), _nhwc(x))
    masked = ref.relu_mask(gy, act)                       # the NumPy mask, not relu_bwd_bias
    _same(_np(gw), ref.conv_weight_grad(x, masked, 1, 1, 1, 3), "conv1_1_backward gw %s" % (case,))
    _same(_np(gb), ref.channel_sums(masked), "conv1_1_backward gb %s" % (case,))


def test_whole_layer_as_the_training_step_chains_it():
    """The masked data gradient of the layer above with its channel sums, then this layer's weight gradient with those sums as bias
    partials: every output against the reference chain."""
    nat = _nat()
    case = cases.CHAIN_CASE
    b, h, w, c = case
    gy2, w2 = cases.dgrad_data(case, (b, h, w, c), (c, 3, 3, c))
    act = cases.activation(case, (b, h, w, c))            # this layer's output = the input of the layer above
    x = cases.ints(np.random.RandomState(7), (b, h, w, c), [-3, -2, -1, 1, 2, 3])
    want_g = ref.conv_input_grad(gy2, w2, (b, h, w, c), 1, 1, 1)
    g, part, masked = _masked_with_sums(_nhwc(gy2), _filters(w2), act, want_g, "chain")
    assert cases.wgrad_exact(b * h * w, max_term=3 * float(np.abs(masked).max()))
    gw, gb = nat.conv3x3_wgrad(_nhwc(x), g, bias_partial=part)
    _same(_np(gw), ref.conv_weight_grad(x, masked, 1, 1, 1, 3), "chain dw")
    _same(_np(gb), ref.channel_sums(masked), "chain db")
