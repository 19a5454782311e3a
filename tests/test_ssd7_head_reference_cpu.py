"""tests/np_ssd7_heads.py against torch's CPU float64 autograd of the two separate head convolutions, and the host arithmetic of the head
weight gradient's plan (ssdhip_ssd7_head_wgrad_plan, csrc/ssdhip_heads7.hip)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import np_ssd7_heads as ref


@pytest.mark.parametrize("cin,b,h,w,nc,nl", [(5, 2, 6, 9, 6, 4), (32, 1, 1, 1, 24, 16), (7, 3, 4, 5, 32, 16), (48, 2, 3, 2, 18, 12)])
def test_reference_equals_torch_autograd(cin, b, h, w, nc, nl):
    rng = np.random.RandomState(cin * 10 + h)
    x, wc, bc, wl, bl, dy = (rng.standard_normal(s) for s in ((b, h, w, cin), (nc, 3, 3, cin), (nc,), (nl, 3, 3, cin), (nl,),
                                                               (b, h, w, ref.CP)))
    nchw = lambda a: torch.from_numpy(a).permute(0, 3, 1, 2)
    xt, wct, wlt = (nchw(a).requires_grad_(True) for a in (x, wc, wl))
    bct, blt = (torch.from_numpy(a).requires_grad_(True) for a in (bc, bl))
    yc, yl = F.conv2d(xt, wct, bct, padding=1), F.conv2d(xt, wlt, blt, padding=1)
    # dL/dy of the packed map: the padding channels carry values too -- nothing of them may reach a gradient
    torch.autograd.backward([yc, yl], [nchw(dy)[:, :nc], nchw(dy)[:, nc:nc + nl]])
    near = lambda got, want: np.abs(got - want.detach().numpy()).max() <= 1e-10
    y = ref.forward(x, wc, bc, wl, bl)
    assert y.shape == (b, h, w, ref.CP)
    assert near(y[..., :nc], yc.permute(0, 2, 3, 1)) and near(y[..., nc:nc + nl], yl.permute(0, 2, 3, 1))
    assert not y[..., nc + nl:].any()
    assert near(ref.input_grad(dy, wc, wl), xt.grad.permute(0, 2, 3, 1))
    dwc, dbc, dwl, dbl = ref.param_grads(x, dy, nc, nl)
    assert near(dwc, wct.grad.permute(0, 2, 3, 1)) and near(dbc, bct.grad)
    assert near(dwl, wlt.grad.permute(0, 2, 3, 1)) and near(dbl, blt.grad)


def _nat():
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd import build
    build.build(verbose=False)
    return nat


def _real_shapes():
    return [(batch, h, w, cin) for batch in (8, 32) for maps in (ref.MAPS_300x300, ref.MAPS_300x480)
            for cin, (h, w) in zip(ref.SOURCES, maps)]


def _test_shapes():
    return [(b, h, w, cin) for cin, b, h, w, _nc, _nl in ref.KERNEL_CASES + ref.SPLIT_CASES]


@pytest.mark.parametrize("b,h,w,cin", _real_shapes() + _test_shapes())
def test_plan_covers_every_position_once_and_fits_its_workspace(b, h, w, cin):
    nat = _nat()
    plan = nat.ssd7_head_wgrad_plan(b, h, w, cin)
    assert plan == nat.ssd7_head_wgrad_plan(b, h, w, cin, 48)                   # the shape alone decides
    splits, per, chunks, last, chunk, rows, parities, positions = plan
    assert positions == ref.padded_list_positions(b, h, w) and chunk == 256 and rows == 3 and parities == (2 if cin == 32 else 1)
    assert chunks == -(-positions // chunk) and 1 <= last <= per and (splits - 1) * per + last == chunks
    seen = np.zeros(chunks * chunk, dtype=np.int64)
    for s in range(splits):
        for c in range(s * per, min((s + 1) * per, chunks)):
            seen[c * chunk:(c + 1) * chunk] += 1
    assert (seen[:positions] == 1).all() and (seen == 1).all()
    # splits: within the operand bytes where that allows eight or more, otherwise eight; at most 64; at most one per chunk
    slot = (48 * 9 * cin + 48) * 4
    operand = b * h * w * (cin + 48) * 2
    assert 1 <= splits <= min(chunks, 64, max(8, operand // (slot * parities)))
    need = int(nat.load().ssdhip_ssd7_head_wgrad_workspace_bytes(b, h, w, cin, 48))
    assert need == splits * parities * slot


def test_plan_refusals_and_the_split_cases():
    nat = _nat()
    lib = nat.load()
    for b, h, w, cin, cp in ((0, 4, 4, 64, 48), (2, 0, 4, 64, 48), (2, 4, 0, 64, 48), (2, 4, 4, 40, 48), (2, 4, 4, 16, 48), (2, 4, 4, 64, 40),
                             (2, 4, 4, 64, 64), (2, 4, 257, 64, 48)):
        assert nat.ssd7_head_wgrad_plan(b, h, w, cin, cp) is None
        assert lib.ssdhip_ssd7_head_wgrad_workspace_bytes(b, h, w, cin, cp) == 0
    for cin, b, h, w, _nc, _nl in ref.SPLIT_CASES:                               # more than one chunk per split, more than one split
        splits, per, chunks, last = nat.ssd7_head_wgrad_plan(b, h, w, cin)[:4]
        assert (splits, per, chunks, last) == (5, 2, 9, 1)
    assert nat.ssd7_head_wgrad_plan(3, 1, 1, 32)[:4] == (1, 1, 1, 1)
    # the 37 x 37 map at batch 32: 48672 positions in 191 chunks, three to a split
    assert nat.ssd7_head_wgrad_plan(32, 37, 37, 64)[:4] == (64, 3, 191, 2)
    assert nat.ssd7_head_geometry(64, 24, 16) and nat.ssd7_head_geometry(32, 32, 16)
    assert not nat.ssd7_head_geometry(64, 84, 16) and not nat.ssd7_head_geometry(128, 24, 16)
