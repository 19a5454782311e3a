"""tests/np_ssd7_conv.py against torch's CPU float64 autograd of F.conv2d, and the host arithmetic of the weight gradient's split plan
(ssdhip_ssd7_conv_wgrad_plan, csrc/ssdhip_wgrad7.hip)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import np_ssd7_conv as ref


@pytest.mark.parametrize("k,cin,cout,b,h,w", [(3, 5, 7, 2, 6, 9), (5, 3, 4, 2, 7, 6), (5, 3, 32, 1, 3, 11), (3, 48, 32, 1, 1, 1)])
def test_reference_equals_torch_autograd(k, cin, cout, b, h, w):
    rng = np.random.RandomState(k * 100 + cin)
    x, wt, bias, dy = (rng.standard_normal(s) for s in ((b, h, w, cin), (cout, k, k, cin), (cout,), (b, h, w, cout)))
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
    wtt = torch.from_numpy(wt).permute(0, 3, 1, 2).requires_grad_(True)
    bt = torch.from_numpy(bias).requires_grad_(True)
    y = F.conv2d(xt, wtt, bt, padding=k // 2)
    y.backward(torch.from_numpy(dy).permute(0, 3, 1, 2))
    near = lambda got, want: np.abs(got - want.detach().numpy()).max() <= 1e-10
    assert near(ref.conv_same(x, wt, bias), y.permute(0, 2, 3, 1))
    assert near(ref.conv_same_input_grad(dy, wt), xt.grad.permute(0, 2, 3, 1))
    dw, db = ref.conv_same_weight_grad(x, dy, k)
    assert near(dw, wtt.grad.permute(0, 2, 3, 1)) and near(db, bt.grad)
    if k == 3:          # the data gradient is the same convolution of dy with the flipped filters
        assert np.abs(ref.conv_same(dy, ref.flipped(wt)) - ref.conv_same_input_grad(dy, wt)).max() <= 1e-10


def _plan(b, h, w, cin, cout, k):
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd import build
    build.build(verbose=False)
    return nat.ssd7_conv_wgrad_plan(b, h, w, cin, cout, k)


@pytest.mark.parametrize("batch", [8, 32])
def test_plan_on_the_real_shapes(batch):
    """Splits cover every tile exactly once, and the partial tiles -- written once, read once -- stay within the operand bytes the launch
    reads (one split, the fewest there are, is exempt: the last maps are smaller than one partial tile)."""
    for (k, cin, cout), (h, w) in zip(ref.LAYERS, ref.MAPS_300x480):
        splits, per, tiles, last = _plan(batch, h, w, cin, cout, k)
        assert tiles == batch * -(-h // 8) * -(-w // 32)
        assert 1 <= splits <= 256 and 1 <= last <= per and (splits - 1) * per + last == tiles
        operand = batch * h * w * (cin + cout) * 2
        partial = splits * (cout * k * k * cin + cout) * 4
        assert splits == 1 or 2 * partial <= operand, (k, cin, cout, splits)
    # block 4 at batch 32 (64 -> 64 on 37 x 60): fewer splits than the part has CUs
    if batch == 32:
        assert _plan(32, 37, 60, 64, 64, 3)[0] < 256


def test_plan_refuses_other_geometries_and_small_cases_split():
    for cin, cout, k in ((40, 48, 3), (32, 40, 3), (3, 32, 3), (32, 48, 5), (48, 32, 1)):
        assert _plan(2, 8, 8, cin, cout, k) is None
    assert _plan(0, 8, 8, 32, 48, 3) is None
    for k, cin, cout in ((3, 32, 48), (5, 3, 32)):         # the GPU tests' several-splits cases
        splits, per, tiles, last = _plan(3, 40, 70, cin, cout, k)
        assert tiles == 45 and splits >= 3 and last < per
    assert _plan(3, 1, 1, 48, 32, 3) == (1, 3, 3, 3)
