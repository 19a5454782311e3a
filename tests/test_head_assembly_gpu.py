"""The prediction assembly (csrc/ssdhip_heads.h head_build_rows through head_kernel; csrc/ssdhip_layers.hip head_grad_kernel) against
the float64 reference tests/np_heads.py, on the cases of tests/head_cases.py: every source path -- float32 packed, packed bf16 by
LDS-DMA, dense bf16, packed bf16 by the gather (for each of its reasons: stride, base alignment, SSDHIP_HEADS_DMA=0, staging size) --
at every tile size, with tiles that start inside a pixel, partial last tiles, 1 to 8 boxes and up to eight layers in one launch.
Needs an MI355X.  One comparison, np_heads.compare_rows: offsets, anchors and variances bit for bit, class probabilities within
(C + 40) 2^-24 of the exact value and within 2e-6.  tests/test_head_reference_cpu.py shows that it rejects one wrong index.

The 2 GB source guard of the LDS-DMA path (src_bytes < 0x7fffff00) cannot be reached at test sizes."""
import numpy as np
import pytest

from tests import head_cases as hc
from tests import np_heads as ref

pytestmark = pytest.mark.gpu


def _t():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from ssd_keras_amd import _native as nat
    return torch, nat


_REF = {}


def _reference(name):
    """(data, anchors, float64 rows) of a case: computed once, shared, never written to."""
    if name not in _REF:
        data, av = hc.case_data(name)
        want = hc.reference(name, data, av)
        want.setflags(write=False)
        _REF[name] = (data, av, want)
    return _REF[name]


def _run(torch, nat, name, data, av, forms=None):
    C, B, av_off, layers, plan, N = hc.case_geometry(name)
    confs, locs, cbs, lbs, nbs = hc.device_heads(torch, C, layers, data, forms)
    y = nat.assemble_predictions(confs, locs, cbs, lbs, nbs, hc.device_anchors(torch, av, av_off), C)
    assert y.shape == (B, N, C + 12) and y.dtype == torch.float32
    return y


@pytest.mark.parametrize("name", list(hc.CASES))
def test_assembly_equals_the_reference_on_every_source_path(name, monkeypatch):
    torch, nat = _t()
    monkeypatch.delenv("SSDHIP_HEADS_DMA", raising=False)
    C, B, av_off, layers, plan, N = hc.case_geometry(name)
    assert hc.plan_of(C, layers, hc.tile_anchors(C)) == plan
    data, av, want = _reference(name)
    y = _run(torch, nat, name, data, av)
    got = y.cpu().numpy()
    assert np.isfinite(got).all()                                          # the NaN padding channels are never read
    print("%s: largest relative error of a class probability %.3g (bound %.3g)" % (name, ref.compare_rows(got, want, C), ref.softmax_rel(C)))
    if name.startswith("f32"):
        return
    # the same logits dense, packed for the LDS-DMA, packed for the gather (tight stride / base off 16 bytes / SSDHIP_HEADS_DMA=0):
    # identical bytes
    n = len(layers)
    for form in ("dense", "dma", "dma8", "tight", "offbase"):
        assert torch.equal(_run(torch, nat, name, data, av, [form] * n), y), form
    monkeypatch.setenv("SSDHIP_HEADS_DMA", "0")
    assert torch.equal(_run(torch, nat, name, data, av, ["dma"] * n), y)
    assert torch.equal(_run(torch, nat, name, data, av), y)


@pytest.mark.parametrize("name,form,dma", [("c21_mixed", "dense", True), ("c21_mixed", "dma", True), ("c21_mixed", "tight", True),
                                           ("c21_mixed", "dma", False), ("f32_c21", None, True), ("c81_coco", "dma8", True),
                                           ("c81_coco", "offbase", True), ("c27_first128", "dense", True)])
def test_non_finite_logits_stay_in_their_row(name, form, dma, monkeypatch):
    """One NaN logit: exactly that anchor's C class columns are NaN, its offsets, its neighbours and the other images untouched.  One
    -inf logit among finite ones: that probability is exactly 0 and the row still sums to 1.  Both sit at a tile seam of the first
    layer: the last anchor of its first tile and the first of its second."""
    torch, nat = _t()
    if dma:
        monkeypatch.delenv("SSDHIP_HEADS_DMA", raising=False)
    else:
        monkeypatch.setenv("SSDHIP_HEADS_DMA", "0")
    C, B, av_off, layers, plan, N = hc.case_geometry(name)
    h, w, nb = layers[0][:3]
    forms = [form] * len(layers) if form else None
    path = hc.source_path(form or layers[0][3], plan[0], C, nb, h * w * nb, dma)
    assert path == {"dense": "D", "dma": "L" if dma else "G", "dma8": "L", "tight": "G", "offbase": "G", None: "F"}[form]
    data0, av, _ = _reference(name)
    data = [dict(d) for d in data0]
    conf = data[0]["conf"].copy().reshape(B, h * w * nb, C)
    b, a_nan, a_inf = B - 1, plan[0] - 1, plan[0]
    conf[b, a_nan, C // 2] = np.nan
    conf[b, a_inf, 1] = -np.inf
    data[0]["conf"] = conf.reshape(data0[0]["conf"].shape)
    want = hc.reference(name, data, av)
    assert np.isnan(want[b, a_nan, :C]).all() and int(np.isnan(want).sum()) == C and want[b, a_inf, 1] == 0.0
    got = _run(torch, nat, name, data, av, forms).cpu().numpy()
    ref.compare_rows(got, want, C)                                          # NaN exactly where the reference has it, 0 exactly where it has 0
    assert np.isnan(got[b, a_nan, :C]).all() and int(np.isnan(got).sum()) == C and got[b, a_inf, 1] == 0.0
    assert abs(float(got[b, a_inf, :C].astype(np.float64).sum()) - 1.0) <= ref.softmax_rel(C)


@pytest.mark.parametrize("name", list(hc.BACKWARD_CASES))
def test_assembly_backward_equals_the_reference(name):
    """head_grad_kernel: 1, 3, 5 and 8 boxes next to 4 and 6, packed strides that are the smallest multiple of 8 as well as multiples
    of 128, C + 12 odd and even with tile starts on every residue mod 4 (tile_copy_f32's unaligned starts).  One bf16 rounding:
    2^-7 |want| + 1e-6; padding exactly zero."""
    torch, nat = _t()
    C, B, maps, nbs, strides, starts = hc.backward_geometry(name)
    assert nat.assemble_backward_supported(C, nbs, strides)
    N = sum(h * w * nb for (h, w), nb in zip(maps, nbs))
    rng = np.random.RandomState(len(name) + C)
    y = np.concatenate([ref.softmax(rng.standard_normal((B, N, C)) * 3), rng.standard_normal((B, N, 4)), rng.random_sample((B, N, 8))], axis=2)
    y = y.astype(np.float32)
    g = rng.standard_normal(y.shape).astype(np.float32)
    want = ref.assemble_backward(g, y, nbs, strides, C, maps)
    got = nat.assemble_predictions_backward(torch.from_numpy(g).cuda(), torch.from_numpy(y).cuda(),
                                            [(B, st, h, w) for (h, w), st in zip(maps, strides)], nbs, C)
    for a, b_, nb, st, (h, w) in zip(got, want, nbs, strides, maps):
        assert a.shape == (B, st, h, w) and a.dtype == torch.bfloat16
        a = a.permute(0, 2, 3, 1).float().cpu().numpy().astype(np.float64)
        assert not a[..., nb * (C + 4):].any()
        err = np.abs(a - b_)
        assert (err <= 2.0 ** -7 * np.abs(b_) + 1e-6).all(), (nb, st, float(err.max()))


def test_refusals_happen_on_the_host():
    """float32 heads with a bias or a separate loc map, a packed map too narrow for its values, a class count beyond the export's
    limit, a ninth layer: refused before any launch."""
    torch, nat = _t()
    C, B, av_off, layers, plan, N = hc.case_geometry("f32_c27")
    data, av, _ = _reference("f32_c27")
    confs, locs, cbs, lbs, nbs = hc.device_heads(torch, C, layers, data)
    avd = hc.device_anchors(torch, av, False)
    bias = torch.zeros((nbs[0] * C,), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(nat.SsdHipError):
        nat.assemble_predictions(confs, locs, [bias] + cbs[1:], lbs, nbs, avd, C)
    with pytest.raises(nat.SsdHipError):
        nat.assemble_predictions(confs, locs, cbs, [bias[:nbs[0] * 4]] + lbs[1:], nbs, avd, C)
    with pytest.raises(nat.SsdHipError):
        nat.assemble_predictions(confs, [confs[0][:, :nbs[0] * 4]] + locs[1:], cbs, lbs, nbs, avd, C)
    narrow = [confs[0].permute(0, 2, 3, 1)[..., :nbs[0] * (C + 4) - 1].contiguous().permute(0, 3, 1, 2)] + confs[1:]
    with pytest.raises(nat.SsdHipError):
        nat.assemble_predictions(narrow, locs, cbs, lbs, nbs, avd, C)
    narrow_bf = [t.to(torch.bfloat16) for t in narrow]
    with pytest.raises(nat.SsdHipError):
        nat.assemble_predictions(narrow_bf, locs, cbs, lbs, nbs, avd, C)
    # the first class count the export refuses, on real tensors
    big = hc.ASSEMBLY_STEPS[-1][0]
    assert hc.tile_anchors(big) == 0 and hc.tile_anchors(big - 1) == 32
    for dt in (torch.bfloat16, torch.float32):
        x = torch.zeros((1, 1, 1, big + 4), dtype=dt, device="cuda").permute(0, 3, 1, 2)
        with pytest.raises(nat.SsdHipError):
            nat.assemble_predictions([x], [None], [None], [None], [1], torch.zeros((1, 8), device="cuda"), big)
    # nine layers (eight run in the case c21_eight)
    x = torch.zeros((1, 1, 1, 32), dtype=torch.bfloat16, device="cuda").permute(0, 3, 1, 2)
    with pytest.raises(nat.SsdHipError):
        nat.assemble_predictions([x] * 9, [None] * 9, [None] * 9, [None] * 9, [1] * 9, torch.zeros((9, 8), device="cuda"), 21)
    y = nat.assemble_predictions([x] * 8, [None] * 8, [None] * 8, [None] * 8, [1] * 8, torch.zeros((8, 8), device="cuda"), 21)
    assert torch.equal(y[..., :21], torch.full((1, 8, 21), 1 / 21, device="cuda"))
