"""ssdhip_decode_from_heads (csrc/ssdhip_decode.hip, scan_heads_kernel: the rows of head_build_rows decoded in LDS) in its 256-, 128-
and 64-thread forms and on every source path.  Needs an MI355X.

(a) Path equality: the same detections, bit for bit, as decoding the assembled tensor -- which shares head_build_rows, so a wrong
    pixel, box or class index in the shared code passes (a).
(b) Planted detections, independent of head_build_rows: anchors on a raster of disjoint cells, background everywhere but at a few
    anchors placed at the seams of the tiling (tests/head_cases.py: plant_sites), each with one class and a distinct logit.  The
    output is known without running project code: which anchors, in which order, with which class, confidence and box."""
import numpy as np
import pytest

from tests import head_cases as hc
from tests import np_heads as ref

pytestmark = pytest.mark.gpu

IMG = 300


def _t():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from ssd_keras_amd import _native as nat
    return torch, nat


def _presentations(name):
    """(forms of every layer or None = the case's own, SSDHIP_HEADS_DMA enabled?)"""
    n = len(hc.CASES[name][3])
    if name.startswith("f32"):
        return [(None, True)]
    return [(None, True), (["dense"] * n, True), (["dma"] * n, True), (["tight"] * n, True), (["dma"] * n, False)]


def _set_dma(monkeypatch, on):
    if on:
        monkeypatch.delenv("SSDHIP_HEADS_DMA", raising=False)
    else:
        monkeypatch.setenv("SSDHIP_HEADS_DMA", "0")


def _params(nat, fast, thresh, normalize):
    """The arguments DecodeDetections / DecodeDetectionsFast pass (keras_layers/): top_k 200, 400 NMS outputs, IoU 0.45."""
    return (thresh, 0.45, 200, 400, fast, nat.SEM_KERAS, "centroids", normalize, IMG if normalize else None, IMG if normalize else None,
            "half", nat.F32, 200)


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("name", hc.DECODE_CASES)
def test_decode_from_heads_equals_assemble_then_decode_at_every_tile_form(name, fast, monkeypatch):
    torch, nat = _t()
    C, B, av_off, layers, plan, N = hc.case_geometry(name)
    assert hc.tile_anchors(C, True) == plan[0] and plan[0] in (64, 128, 256)
    data, av = hc.case_data(name)
    avd = hc.device_anchors(torch, av, av_off)
    want = None
    for forms, dma in _presentations(name):
        _set_dma(monkeypatch, dma)
        confs, locs, cbs, lbs, nbs = hc.device_heads(torch, C, layers, data, forms)
        if want is None:
            want = nat.decode(nat.assemble_predictions(confs, locs, cbs, lbs, nbs, avd, C), *_params(nat, fast, 0.05, True), want_anchor_idx=True)
            assert int(want[1].min()) > 0 and int(want[1].max()) <= 200
        got = nat.decode_from_heads(confs, locs, cbs, lbs, nbs, avd, C, *_params(nat, fast, 0.05, True), want_anchor_idx=True)
        for g, w_, what in zip(got, want, ("out", "count", "anchor_idx")):
            assert g.dtype == w_.dtype and torch.equal(g, w_), (what, forms, dma)


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("name", hc.DECODE_CASES)
def test_planted_detections_come_out_at_their_anchors(name, fast, monkeypatch):
    torch, nat = _t()
    C, B, av_off, layers, plan, N = hc.case_geometry(name)
    data, av = hc.planted_data(name)
    normalize = not fast                                                   # pixel coordinates on one flow, relative ones on the other
    expected = hc.planted_expected(name, IMG if normalize else 1.0)
    avd = hc.device_anchors(torch, av, av_off)
    for forms, dma in _presentations(name):
        _set_dma(monkeypatch, dma)
        confs, locs, cbs, lbs, nbs = hc.device_heads(torch, C, layers, data, forms)
        out, count, aidx = nat.decode_from_heads(confs, locs, cbs, lbs, nbs, avd, C, *_params(nat, fast, hc.planted_threshold(C), normalize),
                                                 want_anchor_idx=True)
        out, count, aidx = out.cpu().numpy(), count.cpu().numpy(), aidx.cpu().numpy()
        assert out.shape == (B, 200, 6) and out.dtype == np.float32
        for b, (rows, idx) in enumerate(expected):
            n = len(idx)
            what = (name, forms, dma, b)
            assert count[b] == n, (what, int(count[b]), n, aidx[b, :count[b]].tolist(), idx.tolist())
            assert np.array_equal(aidx[b, :n], idx), (what, aidx[b, :n].tolist(), idx.tolist())
            assert np.array_equal(out[b, :n, 0], rows[:, 0]), what
            err = np.abs(out[b, :n, 1].astype(np.float64) - rows[:, 1])
            assert (err <= np.minimum(ref.softmax_rel(C) * rows[:, 1], ref.SOFTMAX_ABS)).all(), (what, float(err.max()))
            assert np.array_equal(out[b, :n, 2:].astype(np.float64), rows[:, 2:]), what
            assert not out[b, n:].any() and (aidx[b, n:] == -1).all(), what


def test_decode_from_heads_refuses_tiles_of_fewer_rows_than_a_wave():
    """The first class count whose tile has fewer than 64 anchors (scan_heads_kernel runs one thread per row): SsdHipError from
    decode_from_heads, on the host; the class count before it runs."""
    torch, nat = _t()
    big = hc.DECODE_STEPS[-1][0]
    assert hc.tile_anchors(big, True) == 0 and hc.tile_anchors(big - 1, True) == 64 and hc.tile_anchors(big) == 32
    av = torch.from_numpy(hc.planted_anchors(4).astype(np.float32)).cuda()
    for C, ok in ((big - 1, True), (big, False)):
        x = torch.zeros((1, 1, 1, 4 * (C + 4)), dtype=torch.bfloat16, device="cuda")
        x[..., 5] = 9.0                                                    # anchor 0, class 5
        args = ([x.permute(0, 3, 1, 2)], [None], [None], [None], [4], av, C) + _params(nat, False, 0.5, True)
        if ok:
            out, count, aidx = nat.decode_from_heads(*args, want_anchor_idx=True)
            assert int(count[0]) == 1 and int(aidx[0, 0]) == 0 and float(out[0, 0, 0]) == 5.0
        else:
            with pytest.raises(nat.SsdHipError):
                nat.decode_from_heads(*args)
