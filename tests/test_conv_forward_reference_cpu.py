"""tests/np_conv_forward.py, the float64 statement the inference convolution kernels are compared with, against torch's CPU float64
F.conv2d / F.max_pool2d(ceil_mode=True); every case of tests/forward_exact_cases.py: its data conditions (the share of unit outputs
within +-256; the 2^22 / 2^24 bounds of the float32 sums, the share of outputs that need rounding and the number of ties that
nearest-even and truncation resolve differently for rounding data) and the plan numbers that put it on its seam, from the library's
host-side exports; and the sensitivity of the comparison, shown by mutating the REFERENCE (never a kernel): a dropped term, a dropped
tap of one channel slice, a truncating rounding and a bias added after the rounding must each be reported by `cases.same`."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import forward_exact_cases as cases
from tests import np_conv_forward as ref


def _geometries():
    """Every (k, stride, pad, dilation) the case tables use."""
    geo = set()
    for c in cases.SAME_CASES:
        geo.add((c[5], 1, c[6] * (c[5] // 2), c[6]))
    for c, _ in cases.GENERAL_CASES:
        geo.add((c[5], c[6], c[7], c[8]))
    for c in cases.POOL_CASES:
        geo.add((c[5], 1, c[6] * (c[5] // 2), c[6]))
    for c in cases.SLAB_STRIDED_CASES:
        geo.add((3, c[5], c[6], 1))
    for c in cases.IMAGE_CASES:
        geo.add(c[5:9])
    for c in cases.CHAIN_CASES:
        for l in c[4]:
            geo.add((l[0], l[1], l[2], 1))
    geo.add((3, 1, 1, 1))                                 # the first layer, the resident-filter, block and slab kernels, the groups
    geo.add((1, 1, 0, 1))
    return sorted(geo)


def _torch_conv(x, w, bias, s, p, d):
    y = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2), torch.from_numpy(w).permute(0, 3, 1, 2), None if bias is None else torch.from_numpy(bias), s, p, d)
    return y.permute(0, 2, 3, 1).numpy()


@pytest.mark.parametrize("geo", _geometries())
def test_reference_equals_torch(geo):
    k, s, p, d = geo
    span = d * (k - 1) + 1
    for n, (b, h, w, cin, cout) in enumerate([(2, max(span - 2 * p, 1) + 4, max(span - 2 * p, 1) + 7, 3, 4), (1, max(span - 2 * p, 1), max(span - 2 * p, 1) + 1, 2, 3)]):
        rng = np.random.RandomState(1000 * n + sum(geo))
        x, wt, bias = rng.randn(b, h, w, cin), rng.randn(cout, k, k, cin), rng.randn(cout)
        for bs in (bias, None):
            got = ref.conv_forward(x, wt, bs, s, p, d)
            assert got.shape == (b, ref.out_size(h, s, p, d, k), ref.out_size(w, s, p, d, k), cout)
            np.testing.assert_allclose(got, _torch_conv(x, wt, bs, s, p, d), rtol=0, atol=1e-12)


def test_reference_by_hand():
    """A 2 x 3 one-channel map under a 3 x 3 filter of 1 .. 9 with padding 1: every output worked out by hand; ReLU, the clipped pool
    and the rounding rule on a few numbers."""
    x = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]).reshape(1, 2, 3, 1)
    w = np.arange(1.0, 10.0).reshape(1, 3, 3, 1)
    # y[0, 0] = 5*1 + 6*2 + 8*4 + 9*5 = 94;  y[0, 1] = 4*1 + 5*2 + 6*3 + 7*4 + 8*5 + 9*6 = 154;  y[0, 2] = 4*2 + 5*3 + 7*5 + 8*6 = 106
    # y[1, 0] = 2*1 + 3*2 + 5*4 + 6*5 = 58;  y[1, 1] = 1*1 + 2*2 + 3*3 + 4*4 + 5*5 + 6*6 = 91;   y[1, 2] = 1*2 + 2*3 + 4*5 + 5*6 = 58
    y = ref.conv_forward(x, w, np.array([-100.0]), 1, 1, 1)
    assert y.reshape(2, 3).tolist() == [[-6.0, 54.0, 6.0], [-42.0, -9.0, -42.0]]
    assert ref.relu(y).reshape(2, 3).tolist() == [[0.0, 54.0, 6.0], [0.0, 0.0, 0.0]]
    assert ref.maxpool2_same(y).reshape(-1).tolist() == [54.0, 6.0]                     # windows {(0..1, 0..1)} and the clipped {(0..1, 2)}
    assert ref.conv_forward(np.ones((1, 3, 3, 1)), w, None, 1, 0, 1).reshape(-1).tolist() == [45.0]   # 'valid': one output, the sum of the taps
    # dilation 2 behind padding 2: the rows above and below are outside, column 0 also reads column 2 (tap 6) and column 2 column 0 (tap 4)
    assert ref.conv_forward(x, w, None, 1, 2, 2).reshape(2, 3).tolist() == [[5 + 18.0, 10.0, 4 + 15.0], [20 + 36.0, 25.0, 16 + 30.0]]
    assert ref.conv_forward(x, w, None, 2, 1, 1).reshape(-1).tolist() == [94.0, 106.0]                # stride 2: outputs (0, 0) and (0, 2) of the above
    assert ref.to_bf16(np.array([257.0, 258.0, 259.0, 256.0, 128.5, 129.5, -129.5])).tolist() == [256.0, 258.0, 260.0, 256.0, 128.0, 130.0, -130.0]
    assert cases.bf16_trunc(np.array([257.0, 259.0, 129.5, -129.5])).tolist() == [256.0, 258.0, 129.0, -129.0]
    assert cases.rounding_stats(np.array([257.0, 258.0, 259.0, 129.5, -129.5, 3.0])) == (4 / 6, 3)


@pytest.mark.parametrize("shape", [(2, 5, 7, 3), (1, 1, 1, 2), (2, 4, 6, 2), (1, 3, 2, 4), (3, 1, 5, 1)])
def test_pool_equals_torch_ceil_mode(shape):
    v = np.random.RandomState(sum(shape)).randn(*shape)
    want = F.max_pool2d(torch.from_numpy(v).permute(0, 3, 1, 2), 2, 2, 0, ceil_mode=True).permute(0, 2, 3, 1).numpy()
    got = ref.maxpool2_same(v)
    assert got.shape == (shape[0], (shape[1] + 1) // 2, (shape[2] + 1) // 2, shape[3]) and np.array_equal(got, want)


def test_chain_equals_torch_layer_by_layer_with_one_rounding_per_map():
    rng = np.random.RandomState(5)
    x = ref.to_bf16(rng.randn(2, 9, 8, 4) * 50)
    layers = [dict(w=ref.to_bf16(rng.randn(5, 3, 3, 4)), bias=ref.to_bf16(rng.randn(5)), stride=2, pad=1, dil=1, relu=True),
              dict(w=ref.to_bf16(rng.randn(3, 1, 1, 5)), bias=None, stride=1, pad=0, dil=1, relu=False),
              dict(w=ref.to_bf16(rng.randn(2, 3, 3, 3)), bias=ref.to_bf16(rng.randn(2)), stride=1, pad=0, dil=1, relu=True)]
    got = ref.chain(x, layers)
    cur = x
    for l, y in zip(layers, got):
        want = _torch_conv(cur, l["w"], l["bias"], l["stride"], l["pad"], 1)
        want = np.maximum(want, 0.0) if l["relu"] else want
        np.testing.assert_allclose(y, want, rtol=0, atol=1e-9)
        cur = torch.from_numpy(y).to(torch.bfloat16).double().numpy()                 # torch's own rounding to bf16
        assert np.array_equal(cur, ref.to_bf16(y))
    assert len(got) == 3 and got[2].shape == (2, 3, 2, 2)


# ---- every GPU case: the conditions of its data and the seam of its plan ------------------------------------------------------------
def _check_layer(kind, l, pooled=False, what=""):
    """The conditions of one convolution's data; for rounding data also on the pooled map where the case is compared on one."""
    x, w, bias, pre = l["x"], l["w"], l["bias"], l["pre"]
    assert np.array_equal(ref.to_bf16(x), x) and np.array_equal(ref.to_bf16(w), w) and (bias is None or np.array_equal(ref.to_bf16(bias), bias))
    if kind == "unit":
        assert set(np.unique(x)) <= {-1.0, 1.0} and set(np.unique(w)) <= {-1.0, 1.0}
        assert bias is None or (np.abs(bias).max() <= 3 and not (bias % 1).any())
        assert not (pre % 1).any()
        share = cases.share_within_256(pre)
        print("%s unit: %.4f of the outputs within +-256" % (what, share))
        assert share >= 0.99, (what, share)
        return
    assert not (x % 1).any() and not (w % 1).any() and np.abs(w).max() <= 4 and (bias is None or (np.abs(bias).max() <= 3 and not (bias % 0.5).any()))
    bound = cases.magnitude_bound(x, w, bias, *l["geometry"])
    maps = [cases.epilogue(pre, False), cases.epilogue(pre, True)] + ([cases.epilogue(pre, False, True), cases.epilogue(pre, True, True)] if pooled else [])
    stats = [cases.rounding_stats(m) for m in maps]
    print("%s rounding: sum |x||w| + |bias| <= %d; (share that needs rounding, upward ties) without / with ReLU%s: %s" %
          (what, bound, " and pooled" if pooled else "", stats))
    assert bound < 2 ** 22, (what, bound)
    assert stats[0][0] >= 0.10 and all(s[1] >= 8 for s in stats), (what, stats)
    assert not pooled or stats[2][0] >= 0.10, (what, stats)


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.SAME_CASES)
def test_same_cases(case, kind):
    assert kind != "unit" or case[5] ** 2 * case[3] <= 4608
    _check_layer(kind, cases.same_layer(kind, case), what="same %s" % (case,))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case,plan", cases.GENERAL_CASES)
def test_general_cases(case, plan, kind):
    cases.check_splitk_plan(case, plan)
    _check_layer(kind, cases.general_layer(kind, case), what="general %s" % (case,))


def test_split_k_cases_reach_several_and_uneven_ranges():
    plans = [p for _, p in cases.GENERAL_CASES]
    assert sum(p[1] >= 2 for p in plans) >= 8 and any(p[2] < p[3] for p in plans) and any(p[1] == 12 and p[2] == p[3] for p in plans)
    assert any(p[1] == 1 for p in plans)


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.CIN3_CASES)
def test_first_layer_cases(case, kind):
    l = cases.cin3_layer(kind, case)
    assert kind == "unit" or (l["x"].min() >= 0 and l["x"].max() <= 255)
    _check_layer(kind, l, what="cin3 %s" % (case,))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.POOL_CASES)
def test_pool_cases(case, kind):
    _check_layer(kind, cases.pool_layer(kind, case), pooled=True, what="pool2 %s" % (case,))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("has_bias", [False, True])
@pytest.mark.parametrize("slab", [False, True])
def test_group_cases(slab, has_bias, kind):
    members = cases.group_layers(kind, cases.SLAB_GROUP_SHAPES, has_bias) if slab else cases.group_layers(kind, cases.GROUP_SHAPES, has_bias, cases.GROUP_1X1)
    assert len(members) <= 8 and len({l["x"].shape[1:3] for l in members}) >= 6
    assert not slab or all(l["w"].shape[0] % 128 == 0 and l["x"].shape[2] <= 62 for l in members)
    for i, l in enumerate(members):
        _check_layer(kind, l, what="group member %d %s" % (i, l["x"].shape))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.C64_CASES)
def test_resident_filter_cases(case, kind):
    _check_layer(kind, cases.c64_layer(kind, case), pooled=True, what="c64 %s" % (case,))
    if case == cases.C64_CASES[0]:
        _check_layer(kind, cases.c64_layer(kind, case, False), pooled=True, what="c64 no bias %s" % (case,))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case,plans", cases.SLAB_CASES)
def test_slab_cases(case, plans, kind):
    cases.check_slab_plan(case, False, plans[0])
    cases.check_slab_plan(case, True, plans[1])
    _check_layer(kind, cases.slab_layer(kind, case), pooled=True, what="slab %s" % (case,))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case,plan", cases.SLAB_POOL_CASES)
def test_slab_pool_cases(case, plan, kind):
    cases.check_slab_plan(case, True, plan)
    _check_layer(kind, cases.slab_layer(kind, case), pooled=True, what="slab pooled %s" % (case,))


def test_slab_cases_reach_every_tiling():
    grid = {(5 if c[2] <= 30 else 6 if c[2] <= 62 else 7) for c, p in cases.SLAB_CASES if p[0][0] == 0}
    assert grid == {5, 6, 7}
    assert {p[0][0] for c, p in cases.SLAB_CASES if c[2] > 94} == {4, 5} and any(p[0][0] != 0 and c[2] <= 94 for c, p in cases.SLAB_CASES)
    stacked = [(c, p) for c, p in cases.SLAB_POOL_CASES if p[2]]
    assert {p[2] - c[1] for c, p in stacked} == {1, 2} and {p[0] for c, p in stacked} == {4, 5}          # pitch H + 1 and H + 2; both tile shapes
    assert any(p[2] == (256 >> p[0]) + 2 for c, p in stacked)                                              # the smallest gap: rows of a tile + 2
    assert any(p[1] == c[0] and p[2] == 0 for c, p in cases.SLAB_POOL_CASES)                               # one tile per image
    assert any(c[1] == 2 and c[2] == 2 for c, p in cases.SLAB_POOL_CASES) and any(not c[5] for c, p in cases.SLAB_POOL_CASES)
    # persistent workgroups: tile units = tiles rounded up to 8 x channel tiles; some case sends workgroups to a second tile, plain and pooled
    units = lambda tiles, cout: -(-tiles // 8) * 8 * (cout // 128)
    assert any(units(p[0][1], c[4]) > cases.SLAB_WORKGROUPS and units(p[1][1], c[4]) > cases.SLAB_WORKGROUPS for c, p in cases.SLAB_CASES)
    assert any(units(p[0][1], c[4]) == cases.SLAB_WORKGROUPS for c, p in cases.SLAB_CASES)                  # ... and one fills a round exactly
    assert any(units(-(-c[0] * (c[1] + 1) * (c[2] + 1) // 256), c[4]) > cases.SLAB_WORKGROUPS for c in cases.SLAB_STRIDED_CASES)


def test_resident_filter_and_block_cases_reach_a_second_tile_per_workgroup():
    for table in (cases.C64_CASES, cases.BLOCK_CASES):
        tiles = [cases.c64_tiles(*c[:3]) for c in table]
        assert max(tiles) > cases.C64_WORKGROUPS and 1 in tiles, tiles
    assert cases.c64_tiles(3, 5, 7) == 3 and cases.c64_tiles(40, 16, 16) == 80 and cases.c64_tiles(1, 75, 75) == 50 and cases.c64_tiles(2, 9, 130) == 2 * 17


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.SLAB_STRIDED_CASES)
def test_slab_strided_cases(case, kind):
    assert case[2] <= 94 and case[5] in (1, 2) and case[6] in (0, 1)
    _check_layer(kind, cases.slab_strided_layer(kind, case), what="slab strided %s" % (case,))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.IMAGE_CASES)
def test_image_cases(case, kind):
    b, h, w, cin, cout, k, s, p, d = case
    assert h * w <= 384 and k * k * cin <= 4608
    assert any(c[5] == 1 and c[1] * c[2] > 128 for c in cases.IMAGE_CASES)           # a 1 x 1 layer with more than one 128-pixel tile
    _check_layer(kind, cases.image_layer(kind, case), what="image %s" % (case,))


def _check_chain(kind, ch, kept, what, pooled=False):
    """Layer by layer: operands that are bf16 numbers, sums below 2^24 (2^22 at the last layer, whose bias comes in halves), ref.chain ==
    the builder's maps; unit data: every compared map within +-256 at 99 %; rounding data: every layer's map has ties for the rounding
    between the layers to resolve, the last map needs rounding at 10 % of its outputs."""
    got = ref.chain(ch["x"], ch["layers"])
    for i, (l, m) in enumerate(zip(ch["layers"], ch["maps"])):
        last = i == len(ch["layers"]) - 1
        assert np.array_equal(got[i], m)
        assert np.array_equal(ref.to_bf16(l["w"]), l["w"]) and np.array_equal(ref.to_bf16(l["bias"]), l["bias"])
        assert last or (set(np.unique(l["w"])) <= {-1.0, 0.0, 1.0} and not (l["bias"] % 1).any())
        assert ch["bounds"][i] < (2 ** 22 if last else 2 ** 24), (what, i, ch["bounds"][i])
        if kind == "unit":
            share = cases.share_within_256(ch["pres"][i])
            print("%s unit layer %d: %.4f of the outputs within +-256" % (what, i, share))
            assert (i not in kept and not last) or share >= 0.99, (what, i, share)
        else:
            maps = [m] + ([cases.epilogue(m, True)] if last else []) + ([cases.epilogue(m, r, True) for r in (False, True)] if last and pooled else [])
            stats = [cases.rounding_stats(v) for v in maps]
            print("%s rounding layer %d: sum |x||w| + |bias| <= %d, (share that needs rounding, upward ties) %s" % (what, i, ch["bounds"][i], stats))
            assert all(s[1] >= 8 for s in stats), (what, i, stats)
            assert not last or stats[0][0] >= 0.10, (what, i, stats)


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.BLOCK_CASES)
def test_block_cases(case, kind):
    ch = cases.block_chain(kind, case)
    assert ch["layers"][0]["relu"] and ch["x"].shape[3] == 3 and ch["layers"][0]["w"].shape == (64, 3, 3, 3)
    _check_chain(kind, ch, {1}, "block %s" % (case,), pooled=True)


def test_block_cases_have_a_128_channel_second_layer():
    assert {c[3] for c in cases.BLOCK_CASES} == {64, 128}


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.CHAIN_CASES)
def test_chain_cases(case, kind):
    ch = cases.chain_chain(kind, case)
    _check_chain(kind, ch, {i for i, l in enumerate(case[4]) if l[5]}, "chain %s" % (case[:4],))


# ---- the comparison sees what it is meant to see: mutations of the reference ---------------------------------------------------------
MUTATION_CASE = (2, 19, 19, 128, 128, 3, 1, True)          # 'same' 3 x 3, two channel slices, bias


def _differs(got, want):
    with pytest.raises(AssertionError, match="elements differ, the first at"):
        cases.same(got, want, "mutation")


@pytest.mark.parametrize("kind", cases.KINDS)
def test_comparison_reports_a_dropped_term_and_a_dropped_tap(kind):
    l = cases.layer(kind, ("mutation",) + MUTATION_CASE, MUTATION_CASE[:4], 128, 3, 1, 1, 1, True)
    x, w, pre = l["x"], l["w"], l["pre"]
    ci = 77 + int(np.flatnonzero(x[1, 1, 18, 77:])[0])       # (rounding data has zeros among its x)
    for relu in (False, True):
        want = ref.to_bf16(cases.epilogue(pre, relu))
        # one term -- an input channel under tap (2, 1) -- dropped at the border pixel (0, 18) of image 1 (the tap reads pixel (1, 18))
        lost = pre.copy()
        lost[1, 0, 18, :] -= x[1, 1, 18, ci] * w[:, 2, 1, ci]
        _differs(ref.to_bf16(cases.epilogue(lost, relu)), want)
        if kind == "unit" and not relu:                       # +-1 data: EVERY output channel within +-256 at that pixel sees its lost term
            seen = ref.to_bf16(lost)[1, 0, 18] != want[1, 0, 18]
            assert np.array_equal(seen, np.abs(pre[1, 0, 18]) <= 256) and seen.sum() >= 120
        # the whole tap (0, 2) of the second 64-channel slice dropped everywhere
        w2 = w.copy()
        w2[:, 0, 2, 64:128] = 0
        _differs(ref.to_bf16(cases.epilogue(ref.conv_forward(x, w2, l["bias"], 1, 1, 1), relu)), want)
        # ... and the same term counted twice
        twice = pre.copy()
        twice[1, 0, 18, :] += x[1, 1, 18, ci] * w[:, 2, 1, ci]
        _differs(ref.to_bf16(cases.epilogue(twice, relu)), want)


def test_comparison_reports_a_truncating_store_and_a_late_bias_on_rounding_data():
    l = cases.layer("rounding", ("mutation",) + MUTATION_CASE, MUTATION_CASE[:4], 128, 3, 1, 1, 1, True)
    acc = l["pre"] - l["bias"]
    for relu in (False, True):
        exact = cases.epilogue(l["pre"], relu)
        want = ref.to_bf16(exact)
        _differs(cases.bf16_trunc(exact), want)                                              # truncation instead of round-to-nearest-even
        late = ref.to_bf16(ref.to_bf16(acc) + l["bias"])                                     # the bias added after the rounding (and rounded again)
        _differs(cases.epilogue(late, relu), want)
        # the accumulator kept in bf16 for one step: the last tap's contribution added to a rounded partial sum
        w_last = np.zeros_like(l["w"])
        w_last[:, 2, 2, :] = l["w"][:, 2, 2, :]
        part = ref.conv_forward(l["x"], w_last, None, 1, 1, 1)
        _differs(ref.to_bf16(cases.epilogue(ref.to_bf16(acc - part) + part + l["bias"], relu)), want)


def test_unit_data_is_blind_to_the_rounding_rule_within_256_which_is_why_rounding_data_exists():
    l = cases.layer("unit", ("mutation",) + MUTATION_CASE, MUTATION_CASE[:4], 128, 3, 1, 1, 1, True)
    inside = np.abs(l["pre"]) <= 256
    assert np.array_equal(cases.bf16_trunc(l["pre"])[inside], ref.to_bf16(l["pre"])[inside])
    acc = l["pre"] - l["bias"]
    inside &= np.abs(acc) <= 256
    assert np.array_equal((ref.to_bf16(acc) + l["bias"])[inside], l["pre"][inside])


@pytest.mark.parametrize("kind", cases.KINDS)
def test_pool_before_relu_equals_relu_before_pool(kind):
    """max commutes with ReLU (and with the monotonic rounding): a kernel may pool the accumulators first -- the comparison does not,
    and must not, tell the two orders apart, on a map with negative values either."""
    l = cases.layer(kind, ("mutation",) + MUTATION_CASE, MUTATION_CASE[:4], 128, 3, 1, 1, 1, True)
    pre = l["pre"]
    assert (pre < 0).mean() > 0.3 and (ref.maxpool2_same(pre) < 0).any()
    cases.same(ref.to_bf16(ref.relu(ref.maxpool2_same(pre))), ref.to_bf16(ref.maxpool2_same(ref.relu(pre))), "pool before ReLU")
    cases.same(ref.maxpool2_same(ref.to_bf16(ref.relu(pre))), ref.to_bf16(ref.maxpool2_same(ref.relu(pre))), "pool after the rounding")
    cases.same(ref.to_bf16(ref.maxpool2_same(pre)), ref.maxpool2_same(ref.to_bf16(pre)), "pool after the rounding, no ReLU")
