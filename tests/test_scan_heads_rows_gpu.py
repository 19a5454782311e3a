"""scan_heads_rows_kernel<21> (csrc/ssdhip_decode.hip: decode from the heads with each anchor's row in registers) against
scan_heads_kernel (the rows in LDS), which SSDHIP_SCAN_ROWS=lds forces.  Needs an MI355X.

Every case decodes the same packed bf16 head outputs twice -- forced LDS form, default -- and asks for the same bits: the decoded
boxes (non-finite patterns included), the candidate keys of every (image, class) as sorted multisets (the order inside a list is the
order in which atomics arrive), and the final detections.  Shapes: 3 images, 21 classes, source maps 9x9 with 4 boxes (a full
256-anchor tile and a partial one), 5x5 with 6, 3x3 with 4 and 1x1 with 4 boxes; every map packed [conf | loc | NaN padding] with the
channels rounded up to a multiple of 64, the form the models' head convolutions write and the one that takes the LDS-DMA path.

Rows planted into every layer, at the first and last anchor of every tile among others: all-equal logits, one dominant logit, +inf,
-inf and NaN logits, offsets whose exp overflows, and a confidence exactly at the threshold (class 0 at -30 beside 20 equal classes:
1 / 20 in float32, compared with '>' by the Keras semantics and with '>=' by the class-agnostic NumPy flow).

The class count without an instantiation (6) and separate conf / loc tensors must give what the forced LDS form gives as well: there
the default IS scan_heads_kernel."""
import numpy as np
import pytest

from tests import head_cases as hc

pytestmark = pytest.mark.gpu

IMG = 300
B = 3
MAPS = [(9, 9, 4), (5, 5, 6), (3, 3, 4), (1, 1, 4)]
N = sum(h * w * nb for h, w, nb in MAPS)
T20 = float(np.float32(1.0) / np.float32(20.0))          # the confidence of the threshold rows, a float32 number


def _t():
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU"
    from ssd_keras_amd import _native as nat
    return torch, nat


_DATA = {}


def _data(C, bias, special):
    """Per layer dict(conf, loc, cb, lb) in float64 (bf16 numbers) and anchors_var [N, 8]; built once per (C, bias, special)."""
    key = (C, bias, special)
    if key in _DATA:
        return _DATA[key]
    rng = hc._rng("scan_rows", C, bias)
    data, sites, off = [], [], 0
    for h, w, nb in MAPS:
        conf = hc._grid(rng, (B, h, w, nb * C), 3.0, 11.0)
        loc = hc._grid(rng, (B, h, w, nb * 4), 2.0, 11.0)
        cb = hc._grid(rng, (nb * C,), 1.5, 4.0) if bias else None
        lb = hc._grid(rng, (nb * 4,), 1.5, 4.0) if bias else None
        data.append(dict(conf=conf, loc=loc, cb=cb, lb=lb))
        na = h * w * nb
        local = set()
        for a0 in range(0, na, 256):                           # first, second, middle and last anchors of every tile
            n = min(256, na - a0)
            local |= {a0, a0 + 1, a0 + n // 2, a0 + n - 2, a0 + n - 1}
        sites.append(sorted(a for a in local if 0 <= a < na))
        off += na
    if special:
        kinds = ["equal", "dominant", "pinf", "ninf", "nan", "overflow", "underflow", "thresh", "two_inf"]
        k = 0
        for (h, w, nb), d, ss in zip(MAPS, data, sites):
            conf = d["conf"].reshape(B, h * w * nb, C)
            loc = d["loc"].reshape(B, h * w * nb, 4)
            for a in ss:
                for b in range(B):
                    kind = kinds[k % len(kinds)]
                    k += 1
                    if kind == "equal":
                        conf[b, a, :] = 1.5                              # (equal before the bias: equal logits in the cases without one)
                    elif kind == "dominant":
                        conf[b, a, :] = -8.0
                        conf[b, a, 1 + (a + b) % (C - 1)] = 11.0
                    elif kind == "pinf":
                        conf[b, a, 1 + (a + b) % (C - 1)] = np.inf
                    elif kind == "ninf":
                        conf[b, a, (a + b) % C] = -np.inf
                    elif kind == "nan":
                        conf[b, a, (a + 2 * b) % C] = np.nan
                    elif kind == "overflow":
                        loc[b, a, 2:] = [3.0e4, 2.0e38]
                    elif kind == "underflow":
                        loc[b, a, 2:] = [-3.0e4, -np.inf]
                        loc[b, a, 0] = np.nan
                    elif kind == "thresh" and not bias:
                        conf[b, a, :] = 2.0
                        conf[b, a, 0] = -30.0
                    elif kind == "two_inf":
                        conf[b, a, :] = -np.inf                          # exp(-inf - -inf): a row of NaN
            d["conf"] = conf.reshape(B, h, w, nb * C)
            d["loc"] = loc.reshape(B, h, w, nb * 4)
    rng2 = hc._rng("scan_rows_anchors")
    av = np.empty((N, 8))
    av[:, :2] = rng2.random_sample((N, 2))
    av[:, 2:4] = 0.02 + 0.3 * rng2.random_sample((N, 2))
    av[:, 4:] = [0.1, 0.1, 0.2, 0.2]
    _DATA[key] = (data, av.astype(np.float32).astype(np.float64))
    return _DATA[key]


def _layers(form):
    return [(h, w, nb, form, False, False) for h, w, nb in MAPS]


def _align(v):
    return (v + 255) // 256 * 256


def _run(torch, nat, heads, avd, C, params, agnostic):
    """One decode from the heads: (boxes as uint32 [B, N, 4], per (image, group) the sorted candidate keys, out, count, anchor idx)."""
    out, count, aidx = nat.decode_from_heads(*heads, avd, C, *params, want_anchor_idx=True)
    torch.cuda.synchronize()
    ws = nat.workspaces.get(avd.device, "decode", 0).cpu().numpy()
    G = 1 if agnostic else C - 1
    o_boxes = 0                                                            # csrc/ssdhip_decode.hip, decode_ws_layout
    o_cnt = _align(o_boxes + B * N * 16)
    o_kept_cnt = _align(o_cnt + B * G * 4)
    o_cls = _align(o_kept_cnt + B * G * 4)
    o_cand = _align(o_cls + (B * N * 2 if agnostic else 0))
    boxes = ws[o_boxes:o_boxes + B * N * 16].view(np.uint32).reshape(B, N, 4).copy()
    cnt = ws[o_cnt:o_cnt + B * G * 4].view(np.int32).reshape(B, G).copy()
    cand = ws[o_cand:o_cand + B * G * N * 8].view(np.uint64).reshape(B, G, N)
    assert (cnt >= 0).all() and (cnt <= N).all()
    keys = [[np.sort(cand[b, g, :cnt[b, g]]) for g in range(G)] for b in range(B)]
    return boxes, keys, out.cpu().numpy(), count.cpu().numpy(), aidx.cpu().numpy()


def _same(got, want, what):
    gb, gk, go, gc, gi = got
    wb, wk, wo, wc, wi = want
    assert np.array_equal(gb, wb), (what, "boxes", int((gb != wb).any(axis=2).sum()))
    for b in range(len(wk)):
        for g in range(len(wk[b])):
            assert gk[b][g].shape == wk[b][g].shape and np.array_equal(gk[b][g], wk[b][g]), (what, "keys", b, g, len(gk[b][g]), len(wk[b][g]))
    assert np.array_equal(gc, wc) and np.array_equal(gi, wi), (what, "count / anchors", gc.tolist(), wc.tolist())
    assert go.dtype == wo.dtype and np.array_equal(go.view(np.uint32), wo.view(np.uint32)), (what, "detections")


def _both(monkeypatch, torch, nat, heads, avd, C, params, agnostic, what):
    monkeypatch.setenv("SSDHIP_SCAN_ROWS", "lds")
    want = _run(torch, nat, heads, avd, C, params, agnostic)
    monkeypatch.delenv("SSDHIP_SCAN_ROWS")
    got = _run(torch, nat, heads, avd, C, params, agnostic)
    _same(got, want, what)
    return want


def _params(nat, sem, agnostic, thresh, coords="centroids", normalize=True):
    return (thresh, 0.45, 200, 400, agnostic, sem, coords, normalize, IMG if normalize else None, IMG if normalize else None, "half",
            nat.F32, 200)


# (semantics, class-agnostic, coords, threshold): the Keras layer and its fast twin, the NumPy decoders ('>=' in the class-agnostic one),
# the debug order of the centre decode, both other coordinate forms; the threshold at the planted confidence and away from it
FLOWS = [("keras", False, "centroids", 0.01), ("keras", True, "centroids", 0.01), ("keras", False, "centroids", T20),
         ("keras", True, "centroids", T20), ("numpy", False, "centroids", T20), ("numpy", True, "centroids", T20),
         ("numpy", False, "corners", 0.01), ("numpy", True, "minmax", 0.3), ("debug", False, "centroids", 0.5)]


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("flow", FLOWS, ids=lambda f: "%s-%s-%s-%g" % (f[0], "agnostic" if f[1] else "classes", f[2], f[3]))
def test_rows_in_registers_equal_rows_in_lds(flow, special, bias, monkeypatch):
    torch, nat = _t()
    sem_name, agnostic, coords, thresh = flow
    sem = {"keras": nat.SEM_KERAS, "numpy": nat.SEM_NUMPY, "debug": nat.SEM_DEBUG}[sem_name]
    C = 21
    data, av = _data(C, bias, special)
    layers = [(h, w, nb, "dma", bias, bias) for h, w, nb in MAPS]
    assert hc.plan_of(C, layers, hc.tile_anchors(C, True))[4] == "LLLL"                   # every layer an LDS-DMA layer: the new kernel's case
    heads = hc.device_heads(torch, C, layers, data)
    avd = hc.device_anchors(torch, av, False)
    want = _both(monkeypatch, torch, nat, heads, avd, C, _params(nat, sem, agnostic, thresh, coords), agnostic, flow)
    assert sum(len(k) for img in want[1] for k in img) > 0                               # the comparison is not one of empty lists
    if special:
        assert not np.isfinite(want[0].view(np.float32)).all()                           # the overflowing offsets reached the boxes


def test_threshold_rows_sit_exactly_at_the_threshold(monkeypatch):
    """The planted 1 / 20 confidences: out with '>' (Keras semantics), in with '>=' (class-agnostic NumPy flow), in both forms."""
    torch, nat = _t()
    C = 21
    data, av = _data(C, False, True)
    layers = _layers("dma")
    heads = hc.device_heads(torch, C, layers, data)
    avd = hc.device_anchors(torch, av, False)
    t20_key = np.uint64(int(np.array([T20], dtype=np.float32).view(np.uint32)[0]) | 0x80000000) << np.uint64(20)
    for sem, agnostic, expect in ((nat.SEM_KERAS, False, False), (nat.SEM_NUMPY, True, True)):
        want = _both(monkeypatch, torch, nat, heads, avd, C, _params(nat, sem, agnostic, T20), agnostic, (sem, agnostic))
        at = sum(int(((k >> np.uint64(20)) << np.uint64(20) == t20_key).sum()) for img in want[1] for k in img)
        assert (at > 0) == expect, (sem, agnostic, at)


@pytest.mark.parametrize("what", ["c6", "dense", "dma_off"])
def test_fallbacks_are_the_lds_kernel(what, monkeypatch):
    """No instantiation for 6 classes, separate conf / loc tensors, SSDHIP_HEADS_DMA=0: the default must be scan_heads_kernel."""
    torch, nat = _t()
    C = 6 if what == "c6" else 21
    data, av = _data(C, True, True)
    layers = [(h, w, nb, "dense" if what == "dense" else "dma", True, True) for h, w, nb in MAPS]
    if what == "dma_off":
        monkeypatch.setenv("SSDHIP_HEADS_DMA", "0")
    heads = hc.device_heads(torch, C, layers, data)
    avd = hc.device_anchors(torch, av, False)
    for agnostic in (False, True):
        _both(monkeypatch, torch, nat, heads, avd, C, _params(nat, nat.SEM_KERAS, agnostic, 0.01), agnostic, (what, agnostic))


def test_unaligned_anchors_keep_the_lds_kernel(monkeypatch):
    """anchors_var 4 bytes behind a 16-byte boundary: the float4 anchor loads of the register form do not apply."""
    torch, nat = _t()
    data, av = _data(21, True, True)
    layers = [(h, w, nb, "dma", True, True) for h, w, nb in MAPS]
    heads = hc.device_heads(torch, 21, layers, data)
    avd = hc.device_anchors(torch, av, True)
    _both(monkeypatch, torch, nat, heads, avd, 21, _params(nat, nat.SEM_KERAS, False, 0.01), False, "anchors off alignment")


def test_captured_and_replayed_equals_eager(monkeypatch):
    torch, nat = _t()
    monkeypatch.delenv("SSDHIP_SCAN_ROWS", raising=False)
    C = 21
    data, av = _data(C, True, True)
    layers = [(h, w, nb, "dma", True, True) for h, w, nb in MAPS]
    heads = hc.device_heads(torch, C, layers, data)
    avd = hc.device_anchors(torch, av, False)
    params = _params(nat, nat.SEM_KERAS, False, 0.01)
    eager = [t.clone() for t in nat.decode_from_heads(*heads, avd, C, *params, want_anchor_idx=True)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        nat.decode_from_heads(*heads, avd, C, *params, want_anchor_idx=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        res = nat.decode_from_heads(*heads, avd, C, *params, want_anchor_idx=True)
    torch.cuda.synchronize()
    for _ in range(2):
        for t in res:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for g, w_, name in zip(res, eager, ("out", "count", "anchor_idx")):
            assert torch.equal(g.view(torch.int32), w_.view(torch.int32)), name
