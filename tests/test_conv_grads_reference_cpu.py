"""tests/np_conv_grads.py, the float64 statement the backward kernels are compared with, against torch's CPU float64 autograd of
F.conv2d; and every case of tests/backward_exact_cases.py: its builder's data condition (the 2^24 bound of the float32 sums, the
share of bf16 outputs within +-256) and the plan numbers that put it on its seam, from the library's host-side plan exports."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import backward_exact_cases as cases
from tests import np_conv_grads as ref

# (B, H, W, Cin, Cout, k, stride, pad, dilation): stride 1 / 2 / 3, pad 0 / 1 / 2 / 6, dilation 1 / 2 / 6, rectangular maps, a 1 x 1 map
GEOMETRIES = [
    (2, 5, 7, 3, 4, 3, 1, 1, 1),
    (2, 7, 9, 3, 2, 3, 2, 1, 1),
    (1, 10, 6, 2, 3, 3, 2, 1, 1),
    (2, 5, 8, 3, 2, 3, 1, 0, 1),
    (1, 8, 6, 2, 2, 3, 3, 0, 1),
    (2, 9, 6, 2, 3, 3, 1, 2, 2),
    (1, 7, 5, 2, 2, 3, 1, 6, 6),
    (1, 14, 15, 2, 2, 3, 2, 6, 6),
    (3, 1, 1, 2, 3, 3, 1, 1, 1),
    (2, 1, 1, 3, 2, 3, 1, 6, 6),
    (2, 4, 5, 3, 4, 1, 1, 0, 1),
    (1, 7, 4, 2, 2, 1, 2, 0, 1),
]


@pytest.mark.parametrize("geo", GEOMETRIES)
def test_reference_equals_torch_autograd(geo):
    b, h, w, cin, cout, k, s, p, d = geo
    rng = np.random.RandomState(sum(geo))
    x, wt = rng.randn(b, h, w, cin), rng.randn(cout, k, k, cin)
    dy = rng.randn(b, ref.out_size(h, s, p, d, k), ref.out_size(w, s, p, d, k), cout)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).clone().requires_grad_(True)
    wtt = torch.from_numpy(wt).permute(0, 3, 1, 2).clone().requires_grad_(True)
    y = F.conv2d(xt, wtt, None, s, p, d)
    assert tuple(y.shape) == (b, cout) + dy.shape[1:3]
    (y * torch.from_numpy(dy).permute(0, 3, 1, 2)).sum().backward()
    np.testing.assert_allclose(ref.conv_input_grad(dy, wt, x.shape, s, p, d), xt.grad.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(ref.conv_weight_grad(x, dy, s, p, d, k), wtt.grad.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-12)


def test_data_gradient_is_the_same_convolution_of_the_embedded_gradient_with_flipped_filters():
    """What the training step relies on for the strided and 'valid' 3 x 3 layers: dL/dx = the 3 x 3 'same' convolution of
    embed_strided(dy) with the transposed, tap-flipped filters -- stated here through the reference alone."""
    rng = np.random.RandomState(3)
    for b, h, w, cin, cout, s, p in [(2, 7, 9, 3, 2, 2, 1), (1, 10, 10, 2, 3, 2, 1), (2, 5, 5, 2, 2, 1, 0), (1, 8, 6, 3, 2, 3, 0)]:
        wt = rng.randn(cout, 3, 3, cin)
        dy = rng.randn(b, ref.out_size(h, s, p, 1, 3), ref.out_size(w, s, p, 1, 3), cout)
        z = ref.embed_strided(dy, h, w, s, 1 - p)
        # (the forward 'same' convolution with the transposed, tap-flipped filters IS the input gradient of the 'same' layer with wt)
        same = ref.conv_input_grad(z, wt, (b, h, w, cin), 1, 1, 1)
        np.testing.assert_allclose(same, ref.conv_input_grad(dy, wt, (b, h, w, cin), s, p, 1), rtol=0, atol=1e-12)


def test_small_helpers_by_hand():
    g = np.arange(1.0, 13.0).reshape(1, 2, 3, 2)
    act = np.array([0.0, 1.0, 2.0, 0.0, 0.5, 0.0, 0.0, 0.0, 3.0, 1.0, 0.0, 1.0]).reshape(1, 2, 3, 2)
    m = ref.relu_mask(g, act)
    assert m.reshape(-1).tolist() == [0, 2, 3, 0, 5, 0, 0, 0, 9, 10, 0, 12]
    assert ref.channel_sums(m).tolist() == [17.0, 24.0]
    z = ref.embed_strided(g, 4, 6, 2, 1)
    assert z.shape == (1, 4, 6, 2) and z.sum() == g.sum()
    assert np.array_equal(z[0, 1, 1], g[0, 0, 0]) and np.array_equal(z[0, 3, 5], g[0, 1, 2]) and not z[:, ::2].any() and not z[:, :, ::2].any()
    assert np.array_equal(ref.embed_strided(g, 3, 5, 2, 1)[0, 1, 3], g[0, 0, 1]) and ref.embed_strided(g, 3, 5, 2, 1).sum() == 1 + 2 + 3 + 4
    assert ref.to_bf16(np.array([257.0, 258.0, 259.0, 256.0])).tolist() == [256.0, 258.0, 260.0, 256.0]       # ties to even


# ---- every GPU case: the condition of its data and the seam of its plan ---------------------------------------------------------
@pytest.mark.parametrize("case,plan", cases.WG1_CASES)
def test_1x1_weight_gradient_cases(case, plan):
    b, h, w, cin, cout = case
    cases.check_wg1_plan(case, plan)
    assert cases.wgrad_exact(b * h * w)
    x, dy = cases.wgrad_data(case, (b, h, w, cin), (b, h, w, cout))
    assert np.abs(x).min() == 1 and np.abs(x).max() == 3 and np.abs(dy).min() == 1 and np.abs(dy).max() == 2


def test_more_than_one_split_is_reached_by_some_case_of_each_pixel_gemm():
    assert max(p[1] for _, p in cases.WG1_CASES) >= 3 and max(p[1] for _, p in cases.TAP_CASES) >= 2
    assert any(p[3] < 64 for _, p in cases.WG1_CASES) and any(p[3] == 64 for _, p in cases.WG1_CASES)
    assert any(p[2] < -(-p[0] // p[1]) for _, p in cases.WG1_CASES + cases.TAP_CASES)                  # a short last split


@pytest.mark.parametrize("case,plan", cases.TAP_CASES)
def test_tap_gathered_weight_gradient_cases(case, plan):
    cases.check_tap_plan(case, plan)
    b, ho, wo, _ = cases.tap_out_shape(case)
    assert cases.wgrad_exact(b * ho * wo)


@pytest.mark.parametrize("case,plan", cases.GRID_CASES)
def test_position_grid_weight_gradient_cases(case, plan):
    cases.check_grid_plan(case, plan)
    assert cases.wgrad_exact(case[0] * case[1] * case[2])


@pytest.mark.parametrize("case,plan", cases.DILATED_CASES)
def test_dilated_position_grid_cases(case, plan):
    cases.check_dilated_plan(case, plan)
    assert cases.wgrad_exact(case[0] * case[1] * case[2])


def test_position_grid_cases_reach_every_seam():
    plans = [p for _, p in cases.GRID_CASES]
    assert any(p[3] < p[1] for p in plans)                                          # idle splits
    assert any(p[4] < -(-p[0] // p[1]) for p in plans)                              # a short last split
    assert any(p[1] > 8 for p in plans) and any(p[2] == 2 * p[1] for p in plans)    # split ids beyond one per XCD; the two K halves
    assert {190, 318} <= {c[2] for c, _ in cases.GRID_CASES} and min(c[2] for c, _ in cases.GRID_CASES if c[2] > 1) < 8
    lib = cases._lib()
    assert lib.ssdhip_conv3x3_wgrad_workspace_bytes(1, 3, 191, 64, 128) == 0 and lib.ssdhip_conv3x3_wgrad_workspace_bytes(1, 2, 319, 64, 64) == 0


@pytest.mark.parametrize("case,plan", cases.MASK_CASES)
def test_mask_and_channel_sum_cases(case, plan):
    cases.check_mask_plan(case, plan)


@pytest.mark.parametrize("case,plan", cases.SLAB_CASES)
def test_slab_data_gradient_cases(case, plan):
    cases.check_slab_plan(case, plan)
    b, h, w, cy, cx = case
    assert 9 * cy <= 4608
    if b * h * w * cx > 2 ** 21:                           # (the share of the large case is measured on a slice of its outputs)
        b, cx = 1, 128
    dy, wt = cases.dgrad_data(case, (b, h, w, cy), (cy, 3, 3, cx))
    want = ref.conv_input_grad(dy, wt, (b, h, w, cx), 1, 1, 1)
    assert not (want % 2).any()                            # an even number of +-1 terms everywhere: one lost term makes the sum odd
    assert cases.share_within_256(want) >= 0.99


def test_slab_cases_reach_every_tiling():
    widths = {(p[0], 5 if c[2] <= 30 else 6 if c[2] <= 62 else 7) for c, p in cases.SLAB_CASES if p[0] == 0}
    assert widths == {(0, 5), (0, 6), (0, 7)}
    assert {p[0] for c, p in cases.SLAB_CASES if c[2] > 94} == {4, 5} and any(p[0] != 0 and c[2] <= 94 for c, p in cases.SLAB_CASES)


@pytest.mark.parametrize("case", cases.FORWARD_CASES)
def test_forward_kernel_data_gradient_cases(case):
    b, h, w, cy, cx, k, d, _ = case
    assert k * k * cy <= 4608
    dy, wt = cases.dgrad_data(case, (b, h, w, cy), (cy, k, k, cx))
    want = ref.conv_input_grad(dy, wt, (b, h, w, cx), 1, d * (k // 2), d)
    assert cases.share_within_256(want) >= 0.99


@pytest.mark.parametrize("case", cases.STRIDED_CASES)
def test_strided_and_valid_layer_cases(case):
    """One dy serves the weight gradient (x in +-1..3, dy in +-1, +-2) and the data gradient (w in +-1): its terms are +-1 and +-2, the
    sums stay integers, and the share within +-256 is checked as for the other data gradients."""
    b, h, w, cin, cout, s, p = case
    ho, wo = ref.out_size(h, s, p, 1, 3), ref.out_size(w, s, p, 1, 3)
    assert cases.wgrad_exact(b * ho * wo)
    x, dy = cases.wgrad_data(case, (b, h, w, cin), (b, ho, wo, cout))
    _, wt = cases.dgrad_data(case, (1, 1, 1, 1), (cout, 3, 3, cin))
    assert cases.share_within_256(ref.conv_input_grad(dy, wt, (b, h, w, cin), s, p, 1)) >= 0.99


@pytest.mark.parametrize("case,blocks", cases.FIRST_LAYER_CASES)
def test_first_layer_cases(case, blocks):
    cases.check_first_layer_plan(case, blocks)
    assert cases.wgrad_exact(case[0] * case[1] * case[2])


def test_whole_layer_chain_case():
    """The chain's weight gradient multiplies x in +-1..3 with the bf16 data gradient of the layer above: the float32 bound uses
    that gradient's largest magnitude."""
    b, h, w, c = cases.CHAIN_CASE
    dy, w2 = cases.dgrad_data(cases.CHAIN_CASE, (b, h, w, c), (c, 3, 3, c))
    g = ref.conv_input_grad(dy, w2, (b, h, w, c), 1, 1, 1)
    assert cases.share_within_256(g) == 1.0
    assert cases.wgrad_exact(b * h * w, max_term=3 * float(np.abs(g).max()))
