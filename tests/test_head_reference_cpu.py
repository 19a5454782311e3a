"""No GPU: tests/np_heads.py (the float64 statement of the prediction assembly and of its backward) against torch's CPU float64
softmax and autograd and against a hand-computed case; the sensitivity of its one comparison, compare_rows, to one wrong index; the
plans and data conditions of every case of tests/head_cases.py, recomputed from the library's export; and the host-side refusals of
the assembly entries."""
import ctypes

import numpy as np
import pytest

from tests import head_cases as hc
from tests import np_heads as ref


# ---- the tile arithmetic, from the export -------------------------------------------------------------------------------------------
def test_tile_steps_are_what_the_export_reports():
    assert hc.tile_steps(False) == hc.ASSEMBLY_STEPS
    assert hc.tile_steps(True) == hc.DECODE_STEPS
    assert hc.tile_anchors(1) == 0 and hc.tile_anchors(1025) == 0 and hc.tile_anchors(0, True) == 0 and hc.tile_anchors(-3) == 0


@pytest.mark.parametrize("name", list(hc.CASES))
def test_case_reaches_its_seams(name):
    C, B, av_off, layers, plan, N = hc.case_geometry(name)
    assert B in (1, 3) and 1 <= len(layers) <= hc.MAX_LAYERS
    assert hc.plan_of(C, layers, hc.tile_anchors(C)) == plan, hc.plan_of(C, layers, hc.tile_anchors(C))
    assert all(h * w * nb <= 300 for h, w, nb, *_ in layers)
    # with SSDHIP_HEADS_DMA=0 every packed bf16 layer gathers
    off = hc.plan_of(C, layers, hc.tile_anchors(C), dma_enabled=False)[4]
    assert "L" not in off and off == plan[4].replace("L", "G")
    if name in hc.DECODE_CASES:
        assert hc.tile_anchors(C, True) == plan[0]


def test_the_table_covers_every_seam_the_tiling_has():
    by_ta = {}
    for name in hc.CASES:
        C, B, av_off, layers, plan, N = hc.case_geometry(name)
        by_ta.setdefault(plan[0], []).append((name, C, B, av_off, layers, plan))
    assert sorted(by_ta) == [32, 64, 128, 256]
    first = {ta: c for c, ta in hc.ASSEMBLY_STEPS}
    for ta, cases in by_ta.items():
        layers = [l for c in cases for l in c[4]]
        bf = [l for c in cases if not c[0].startswith("f32") for l in c[4]]
        assert any(ta % nb and h * w * nb > ta and (h * w * nb) % ta for h, w, nb, *_ in bf), ta      # a tile starts and ends inside a pixel, partial last tile
        assert any(h * w * nb == ta for h, w, nb, *_ in layers), ta
        assert any(h * w == 1 for h, w, *_ in layers), ta
        assert any(c[0].startswith("f32") for c in cases), ta
        paths = "".join(c[5][4] for c in cases)
        assert set(paths) == set("DLGF"), (ta, paths)
        # both sides of the step: the first class count of this tile size and the last before the next
        cs = {c[1] for c in cases}
        nxt = min(c for c, t in hc.ASSEMBLY_STEPS if c > first[ta])
        assert first[ta] in cs or ta == 256, (ta, cs)
        assert nxt - 1 in cs, (ta, cs)
    allc = {hc.CASES[n][0] for n in hc.CASES}
    assert {2, 6, 21, 81} <= allc
    assert {c % 4 for c in allc if not isinstance(c, str)} == {0, 1, 2, 3}
    every = [(n, l) for n in hc.BF16_CASES for l in hc.CASES[n][3]]
    assert {l[2] for _, l in every} >= {1, 3, 4, 5, 6, 8}
    assert {(l[4], l[5]) for _, l in every} == {(True, True), (True, False), (False, True), (False, False)}
    assert {hc.CASES[n][2] for n in hc.BF16_CASES} == {True, False}
    # each reason for the gather: a stride off a multiple of 8, a base off 16 bytes, the staging size alone
    assert any(l[3] == "tight" and hc.stride_of("tight", l[2], hc.CASES[n][0]) % 8 for n, l in every)
    assert any(l[3] == "offbase" for n, l in every)
    C, B, av_off, layers, plan, N = hc.case_geometry("c61_staging")
    h, w, nb, form, _, _ = layers[0]
    assert hc.stride_of(form, nb, C) % 8 == 0 and form == "dma8" and plan[4][0] == "G" and not hc.staging_fits(plan[0], C, nb, h * w * nb)
    assert any(len(hc.CASES[n][3]) == hc.MAX_LAYERS for n in hc.CASES)
    # an anchors-of-the-AV16-branch case takes the DMA path at all
    assert any(hc.CASES[n][2] and "L" in hc.CASES[n][4][4] for n in hc.BF16_CASES)


def test_staging_size_alone_sends_only_large_box_counts_to_the_gather():
    """Host arithmetic over every accepted class count and every tile origin: the staging-size condition of the LDS-DMA path fails for
    no layer of fewer than 14 boxes per pixel (the models have at most 6), and does fail beyond."""
    fails = set()
    for C in range(2, 243):
        ta = hc.tile_anchors(C)
        for nb in range(1, 41):
            if not hc.staging_fits(ta, C, nb, ta * nb):           # every alignment of a tile against the pixels
                fails.add(nb)
    assert fails and min(fails) == 14, sorted(fails)[:5]


@pytest.mark.parametrize("name", list(hc.CASES))
def test_case_data_conditions(name):
    C, B, av_off, layers, plan, N = hc.case_geometry(name)
    data, av = hc.case_data(name)
    assert av.shape == (N, 8) and np.isfinite(av).all() and np.array_equal(av.astype(np.float32).astype(np.float64), av)
    for d, (h, w, nb, form, has_cb, has_lb) in zip(data, layers):
        assert (d["cb"] is not None) == has_cb and (d["lb"] is not None) == has_lb
        for k, bias in (("conf", d["cb"]), ("loc", d["lb"])):
            x = d[k]
            assert np.isfinite(x).all()
            if form in ("f32", "f32t"):
                assert bias is None and np.array_equal(x.astype(np.float32).astype(np.float64), x)
            else:
                assert ref.is_bf16(x) and np.array_equal(np.rint(x * 64), x * 64)
                if bias is not None:
                    assert ref.is_bf16(bias) and np.array_equal(np.rint(bias * 64), bias * 64)
                    s = x.reshape(B, h, w, nb, -1) + bias.reshape(nb, -1)
                    assert np.array_equal(s.astype(np.float32).astype(np.float64), s)          # the float32 sum is exact
                    x = ref.bf16_round(s)
            if k == "conf":
                assert np.abs(x).max() <= 16
    want = hc.reference(name, data, av)
    assert want.shape == (B, N, C + 12) and np.isfinite(want).all()


@pytest.mark.parametrize("name", hc.DECODE_CASES)
def test_planted_detections_are_separable(name):
    C, B, av_off, layers, plan, N = hc.case_geometry(name)
    pl = hc.planted(name)
    sites = hc.plant_sites(layers, plan[0])
    offs = np.cumsum([0] + [h * w * nb for h, w, nb, *_ in layers])
    assert {int(o) for o in offs[:-1]} <= set(sites) and {int(o) - 1 for o in offs[1:]} <= set(sites)
    assert any(a % plan[0] == plan[0] - 1 for a in sites) and len(sites) > 2 * len(layers)
    per_image = [sorted(a for b, a, c, s in pl if b == i) for i in range(B)]
    assert all(len(p) >= 4 for p in per_image) and (B == 1 or per_image[0] != per_image[1] != per_image[2])
    for i in range(B):
        logits = [s for b, a, c, s in pl if b == i]
        assert len(set(logits)) == len(logits) and all(2 <= s <= 12 and ref.is_bf16(s) for s in logits)
    classes = {c for b, a, c, s in pl}
    assert 1 in classes and C - 1 in classes and 0 not in classes
    thr = hc.planted_threshold(C)
    assert 1 / (np.exp(8) + C - 1) < 3.4e-4 < 1 / (np.exp(2) + C - 1) < thr < np.exp(2) / (np.exp(2) + C - 1)
    # the expected rows against the reference on the planted data: the only use of project-independent arithmetic twice
    data, av = hc.planted_data(name)
    y = ref.assemble([d["conf"] for d in data], [d["loc"] for d in data], None, None, [l[2] for l in layers], av, C,
                     src="f32" if name.startswith("f32") else "bf16")
    exp = hc.planted_expected(name, 1.0)
    for i, (rows, idx) in enumerate(exp):
        assert np.all(np.diff(rows[:, 1]) < -4e-5)
        for r, a in zip(rows, idx):
            assert abs(y[i, a, int(r[0])] - r[1]) < 1e-13 and np.array_equal(y[i, a, C + 4:C + 8], av[a, :4])
        assert int((y[i, :, 1:C] > thr).sum()) == len(idx)
    boxes = exp[0][0][:, 2:]
    assert (boxes[:, 2] > boxes[:, 0]).all() and len({tuple(b) for b in boxes}) == len(boxes)


# ---- the reference itself -----------------------------------------------------------------------------------------------------------
def test_bf16_round_is_round_to_nearest_even():
    import torch
    x = np.concatenate([np.random.RandomState(3).standard_normal(4000) * 37, [0.0, 1.00390625, 1.01171875, -1.00390625, 3.0 * 2.0 ** -130,
                                                                               2.0 ** -134, 255.5, 256.5, 1e-40, np.inf, -np.inf]])
    x = x.astype(np.float32).astype(np.float64)
    want = torch.from_numpy(x.astype(np.float32)).to(torch.bfloat16).double().numpy()
    assert np.array_equal(ref.bf16_round(x), want)
    assert ref.bf16_round(1.00390625) == 1.0 and ref.bf16_round(1.01171875) == 1.015625         # ties: to the even neighbour
    assert np.isnan(ref.bf16_round(np.nan))


@pytest.mark.parametrize("name", ["c21_mixed", "c27_first128", "c2_smallest", "f32_c21", "c21_eight"])
def test_assemble_equals_torch_float64(name):
    import torch
    C, B, av_off, layers, plan, N = hc.case_geometry(name)
    data, av = hc.case_data(name)
    f32 = name.startswith("f32")
    zs, ls = [], []
    for d, (h, w, nb, *_) in zip(data, layers):
        z, lo = torch.from_numpy(d["conf"]), torch.from_numpy(d["loc"])
        if not f32:                                              # the framework's bf16 bias add
            z, lo = z.to(torch.bfloat16), lo.to(torch.bfloat16)
            if d["cb"] is not None:
                z = z + torch.from_numpy(d["cb"]).to(torch.bfloat16)
            if d["lb"] is not None:
                lo = lo + torch.from_numpy(d["lb"]).to(torch.bfloat16)
        zs.append(z.double().reshape(B, -1, C))
        ls.append(lo.double().reshape(B, -1, 4))
    want = torch.cat([torch.softmax(torch.cat(zs, 1), -1), torch.cat(ls, 1), torch.from_numpy(av).unsqueeze(0).expand(B, -1, -1)], 2).numpy()
    got = hc.reference(name, data, av)
    assert np.array_equal(got[..., C:], want[..., C:])
    np.testing.assert_allclose(got[..., :C], want[..., :C], rtol=1e-13, atol=0)
    # the packed layout of the same values (padding NaN) is the same rows
    packed = [hc.packed_array(d["conf"], d["loc"], d["conf"].shape[3] + d["loc"].shape[3] + 5) for d in data]
    again = ref.assemble(packed, [None] * len(data), [d["cb"] for d in data], [d["lb"] for d in data], [l[2] for l in layers], av, C,
                         src="f32" if f32 else "bf16")
    assert np.array_equal(again, got)


def test_assemble_hand_case():
    """Two anchors (one pixel, two boxes), three classes.  Logits (0, ln 2, ln 5) -> 1/8, 2/8, 5/8; the second box gets its bias:
    (1, 1, 1) + (0, 0, ln 3 rounded to bf16 = 1.1015625) rounds to (1, 1, 2.09375)."""
    l2, l5 = ref.bf16_round(np.log(2.0)), ref.bf16_round(np.log(5.0))
    conf = np.array([0.0, l2, l5, 1.0, 1.0, 1.0]).reshape(1, 1, 1, 6)
    loc = np.array([0.5, -1.0, 2.0, 4.0, -0.25, 0.0, 1.0, 8.0]).reshape(1, 1, 1, 8)
    cb = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 1.1015625])
    lb = np.array([0.0, 0.0, 0.0, 0.0, 0.25, 0.0, 0.0, 0.03125])
    av = np.arange(16, dtype=np.float64).reshape(2, 8) / 16
    y = ref.assemble([conf], [loc], [cb], [lb], [2], av, 3)
    e = np.exp([0.0, l2, l5])
    assert y.shape == (1, 2, 15)
    np.testing.assert_allclose(y[0, 0, :3], e / e.sum(), rtol=1e-15)
    np.testing.assert_allclose(y[0, 0, :3], [1 / 8, 2 / 8, 5 / 8], rtol=4e-3)                     # (the logits are bf16 roundings of ln 2, ln 5)
    assert ref.bf16_round(2.1015625) == 2.09375
    t = np.exp(2.09375 - 1.0)
    np.testing.assert_allclose(y[0, 1, :3], [1 / (2 + t), 1 / (2 + t), t / (2 + t)], rtol=1e-15)
    assert y[0, 0, 3:7].tolist() == [0.5, -1.0, 2.0, 4.0]
    assert y[0, 1, 3:7].tolist() == [0.0, 0.0, 1.0, 8.0]                                         # 8 + 2^-5 rounds back to 8
    assert np.array_equal(y[0, :, 7:], av)
    # backward by hand: g = e_0 on anchor 0 -> p_0 (1 - p_0), -p_1 p_0, -p_2 p_0; offsets pass; padding zero
    g = np.zeros((1, 2, 15))
    g[0, 0, 0] = 1.0
    g[0, 1, 3:7] = [1, 2, 3, 4]
    g[0, :, 7:] = 9.0                                                                            # no producer: dropped
    (d,) = ref.assemble_backward(g, y, [2], [16], 3, [(1, 1)])
    p = y[0, 0, :3]
    np.testing.assert_allclose(d[0, 0, 0, :3], [p[0] * (1 - p[0]), -p[1] * p[0], -p[2] * p[0]], rtol=1e-15)
    assert d[0, 0, 0, 3:6].tolist() == [0, 0, 0] and d[0, 0, 0, 6:14].tolist() == [0, 0, 0, 0, 1, 2, 3, 4] and d[0, 0, 0, 14:].tolist() == [0, 0]


@pytest.mark.parametrize("name", list(hc.BACKWARD_CASES))
def test_assemble_backward_equals_float64_autograd(name):
    import torch
    C, B, maps, nbs, strides, starts = hc.backward_geometry(name)
    assert sorted({s % 4 for s in starts}) == list(hc.BACKWARD_CASES[name][3])
    assert all(st % 8 == 0 and st >= nb * (C + 4) for st, nb in zip(strides, nbs))
    rng = np.random.RandomState(5)
    packed = [torch.from_numpy(rng.standard_normal((B, h, w, st)) * 3).requires_grad_(True) for (h, w), st in zip(maps, strides)]
    zs = [p[..., :nb * C].reshape(B, -1, C) for p, nb in zip(packed, nbs)]
    ls = [p[..., nb * C:nb * (C + 4)].reshape(B, -1, 4) for p, nb in zip(packed, nbs)]
    N = sum(h * w * nb for (h, w), nb in zip(maps, nbs))
    av = torch.from_numpy(rng.random_sample((N, 8)))
    y = torch.cat([torch.softmax(torch.cat(zs, 1), -1), torch.cat(ls, 1), av.unsqueeze(0).expand(B, -1, -1)], 2)
    g = torch.from_numpy(rng.standard_normal(tuple(y.shape)))
    want = torch.autograd.grad((y * g).sum(), packed)
    got = ref.assemble_backward(g.numpy(), y.detach().numpy(), nbs, strides, C, maps)
    for a, b_, nb in zip(got, want, nbs):
        np.testing.assert_allclose(a, b_.numpy(), rtol=1e-11, atol=1e-15)
        assert not a[..., nb * (C + 4):].any()


def test_backward_table_covers_box_counts_strides_and_unaligned_tile_starts():
    nbs, res, kinds, par = set(), set(), set(), set()
    for name, (C, B, layers, residues) in hc.BACKWARD_CASES.items():
        nbs |= {l[2] for l in layers}
        kinds |= {l[3] for l in layers}
        res |= set(residues)
        par.add((C + 12) % 2)
        assert B in (1, 3) and all(h * w * nb <= 300 for h, w, nb, _ in layers)
        assert any(h * w * nb > hc.HG_TILE for h, w, nb, _ in layers)              # more than one tile
    assert nbs >= {1, 3, 4, 5, 6, 8} and res == {0, 1, 2, 3} and kinds == {"8", "128"} and par == {0, 1}


# ---- compare_rows sees one wrong index ----------------------------------------------------------------------------------------------
def _rejected(got, want, C):
    with pytest.raises(AssertionError):
        ref.compare_rows(got, want, C)


@pytest.mark.parametrize("name", list(hc.CASES))
def test_compare_rows_rejects_one_planted_error(name):
    C, B, av_off, layers, plan, N = hc.case_geometry(name)
    want = hc.reference(name)
    good = want.astype(np.float32)
    assert ref.compare_rows(good, want, C) <= 2.0 ** -24                   # the rounded reference passes
    offs = np.cumsum([0] + [h * w * nb for h, w, nb, *_ in layers])
    # two boxes of one pixel swapped: the last pixel of the first layer with more than one box
    li = next(i for i, l in enumerate(layers) if l[2] > 1)
    nb = layers[li][2]
    a = int(offs[li + 1]) - nb
    bad = good.copy()
    bad[:, [a, a + nb - 1]] = good[:, [a + nb - 1, a]]
    assert not np.array_equal(good[:, a], good[:, a + nb - 1])
    _rejected(bad, want, C)
    # ... judged by the class columns alone (the offsets and anchors put right)
    bad[:, [a, a + nb - 1], C:] = good[:, [a, a + nb - 1], C:]
    assert not np.array_equal(bad[:, a, :C], good[:, a, :C])
    _rejected(bad, want, C)
    # two classes of one row swapped: the likeliest and the least likely one
    row = good[B - 1, N // 2, :C]
    i, j = int(row.argmax()), int(row.argmin())
    bad = good.copy()
    bad[B - 1, N // 2, [i, j]] = row[[j, i]]
    assert row[i] != row[j]
    _rejected(bad, want, C)
    # ... and two neighbouring classes of every row, by the class columns alone
    if C > 2:
        bad = good.copy()
        bad[..., [1, 2]] = good[..., [2, 1]]
        assert not np.array_equal(bad, good)
        _rejected(bad, want, C)
    # one anchor shifted by one (the first anchor of the second tile reads the row before it)
    a = min(plan[0], N - 1)
    bad = good.copy()
    bad[:, a] = good[:, a - 1]
    assert not np.array_equal(good[:, a], good[:, a - 1])
    _rejected(bad, want, C)
    bad[:, a, C:] = good[:, a, C:]                                          # ... in the class columns only
    assert not np.array_equal(bad[:, a, :C], good[:, a, :C])
    _rejected(bad, want, C)
    # one offset off by one bf16 ulp (float32 heads: one float32 ulp)
    bad = good.copy()
    v = bad[0, N - 1, C + 2]
    bad[0, N - 1, C + 2] = np.nextafter(v, np.float32(np.inf)) if name.startswith("f32") else np.float32(v + max(abs(v), 2.0 ** -126) * 2.0 ** -7)
    assert bad[0, N - 1, C + 2] != v
    _rejected(bad, want, C)
    # one anchor's row taken from the neighbouring image
    if B > 1:
        bad = good.copy()
        bad[1, 3] = good[2, 3]
        assert not np.array_equal(good[1, 3], good[2, 3])
        _rejected(bad, want, C)
        bad[1, 3, C:] = good[1, 3, C:]
        assert not np.array_equal(bad[1, 3, :C], good[1, 3, :C])
        _rejected(bad, want, C)
    # an anchor / variance column of the neighbouring anchor
    bad = good.copy()
    bad[0, 0, C + 4:] = good[0, 1, C + 4:]
    _rejected(bad, want, C)


def test_compare_rows_on_non_finite_rows():
    z = np.array([[[0.0, 1.0, -np.inf], [0.0, np.nan, 1.0]]]).reshape(1, 1, 2, 3)
    want = ref.assemble([z], [np.zeros((1, 1, 2, 4))], None, None, [1], np.ones((2, 8)), 3)
    assert want[0, 0, 2] == 0.0 and abs(want[0, 0, :3].sum() - 1) < 1e-15 and np.isnan(want[0, 1, :3]).all() and np.isfinite(want[0, 1, 3:]).all()
    good = want.astype(np.float32)
    ref.compare_rows(good, want, 3)
    bad = good.copy()
    bad[0, 0, 2] = 1e-30                                                   # exp(-inf) is exactly 0
    _rejected(bad, want, 3)
    bad = good.copy()
    bad[0, 1, 0] = 0.3                                                     # a NaN logit makes every class of its row NaN
    _rejected(bad, want, 3)
    bad = good.copy()
    bad[0, 0, 0] = np.nan
    _rejected(bad, want, 3)


# ---- host-side refusals (no launch: callable without a GPU) ---------------------------------------------------------------------------
def test_assembly_entries_refuse_a_tile_beyond_one_launch_on_the_host():
    """head_kernel gets head_tile_lds(32, C) bytes of dynamic LDS without an opt-in: from C = 243 that exceeds 64 KB.  Both assembly
    entries return SSDHIP_E_BADARG before any launch, and the export reports 0; C = 242 is the last class count they take."""
    from ssd_keras_amd import _native as nat
    lib = nat.load()
    first_refused = hc.ASSEMBLY_STEPS[-1][0]
    assert hc.tile_anchors(first_refused) == 0 and hc.tile_anchors(first_refused - 1) == 32
    assert 32 * (6 * first_refused + 72) + 64 * first_refused + 1280 > 64 * 1024 >= 32 * (6 * (first_refused - 1) + 72) + 64 * (first_refused - 1) + 1280
    dummy = ctypes.create_string_buffer(64)
    a = ctypes.addressof(dummy)
    a += (-a) % 16                                                         # a non-null fake pointer (never dereferenced)
    one = lambda v: (ctypes.c_void_p * 1)(v)
    ints = lambda *v: (ctypes.c_int * len(v))(*v)
    for C in (first_refused, 300, 1024, 1025, 1):
        assert hc.tile_anchors(C) == 0                                     # (the calls below would launch otherwise)
        assert lib.ssdhip_assemble_predictions_strided_bf16(1, one(a), one(a), one(None), one(None), ints(4), ints(4), ints(4 * (C + 4)),
                                                            ints(4 * (C + 4)), a, 1, 4, C, a, None) == -1, C
        assert lib.ssdhip_assemble_predictions_strided_f32(1, one(a), one(a), ints(4), ints(4), ints(4 * (C + 4)), ints(4 * (C + 4)), a, 1, 4,
                                                           C, a, None) == -1, C
        assert lib.ssdhip_assemble_predictions_bf16(1, one(a), one(a), one(None), one(None), ints(4), ints(4), a, 1, 4, C, a, None) == -1, C
    # layers 8 and 9: nine are refused whatever else holds (eight run in tests/test_head_assembly_gpu.py)
    for n in (hc.MAX_LAYERS + 1, hc.MAX_LAYERS + 2):                       # a ninth and a tenth layer (indices 8 and 9)
        ptrs = (ctypes.c_void_p * n)(*[a] * n)
        nulls = (ctypes.c_void_p * n)(*[None] * n)
        rep = lambda v: (ctypes.c_int * n)(*[v] * n)
        assert lib.ssdhip_assemble_predictions_strided_bf16(n, ptrs, ptrs, nulls, nulls, rep(4), rep(4), rep(100), rep(100), a, 1, 4 * n, 21, a,
                                                            None) == -1
        assert lib.ssdhip_assemble_predictions_strided_f32(n, ptrs, ptrs, rep(4), rep(4), rep(100), rep(100), a, 1, 4 * n, 21, a, None) == -1
