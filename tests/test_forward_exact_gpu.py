"""The inference convolution kernels (csrc/ssdhip_conv.hip, ssdhip_conv64.hip, ssdhip_convh.hip, ssdhip_convimg.hip, ssdhip_chain.hip)
against tests/np_conv_forward.py (float64) on data where float32 accumulation is exact in any order (tests/forward_exact_cases.py):
every comparison is equality of values with the float64 result rounded ONCE to bf16 -- no other kernel, no tolerance, no cap on
differing elements.  "unit" data (+-1 operands, integer bias) shows one dropped, doubled or misplaced term of a sum over taps, K slices,
K ranges or tiles; "rounding" data (wider integers, a bias in halves) shows a truncating store, a bias added after the rounding, a
double rounding.  Every entry runs without ReLU (full sensitivity) and with it; pooled outputs are the maximum of the exact values
rounded once; pool_keep entries are compared on both maps, grouped launches on every member, chain and block kernels on every kept
map.  An entry that returns None for a case of the tables fails the test: the geometry must be supported.  Needs an MI355X."""
import numpy as np
import pytest

from tests import forward_exact_cases as cases
from tests import np_conv_forward as ref

pytestmark = pytest.mark.gpu

RELU = (False, True)


def _nat():
    from ssd_keras_amd import _native as nat
    return nat


def _nhwc(a):
    """[N, H, W, C] float64 array of bf16 values -> (N, C, H, W) bf16 CUDA tensor with NHWC memory (a map, or [Cout, k, k, Cin] filters)."""
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(torch.bfloat16).cuda().permute(0, 3, 1, 2)      # (a copy: the cached arrays are read-only)


def _vec(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, dtype=np.float64)).to(torch.bfloat16).cuda()


def _np(t):
    """A device map as float64 in NHWC order."""
    assert t is not None, "geometry must be supported"
    return t.detach().double().cpu().permute(0, 2, 3, 1).numpy()


def _upload(l):
    """The operands of cases.layer() on the device; the upload must not have changed a value (they are bf16 numbers by construction)."""
    xd, wd, bd = _nhwc(l["x"]), _nhwc(l["w"]), _vec(l["bias"])
    assert np.array_equal(_np(xd), l["x"]) and np.array_equal(_np(wd), l["w"])
    assert bd is None or np.array_equal(bd.double().cpu().numpy(), l["bias"])
    return xd, wd, bd


def _want(l, relu, pool=False):
    return ref.to_bf16(cases.epilogue(l["pre"], relu, pool))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.SAME_CASES)
def test_same_convolution_every_variant(case, kind):
    nat = _nat()
    l = cases.same_layer(kind, case)
    xd, wd, bd = _upload(l)
    for relu in RELU:
        want = _want(l, relu)
        for variant in cases.SAME_VARIANTS:
            got = nat.conv2d_same(xd, wd, bd, dilation=case[6], relu=relu, variant=variant)
            cases.same(_np(got), want, "conv2d_same %s %s variant %s relu %s" % (case, kind, variant, relu))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case,plan", cases.GENERAL_CASES)
def test_general_convolution_every_variant_and_split_k(case, plan, kind):
    nat = _nat()
    cases.check_splitk_plan(case, plan)
    s, p, d = case[6:9]
    l = cases.general_layer(kind, case)
    xd, wd, bd = _upload(l)
    for relu in RELU:
        want = _want(l, relu)
        for variant in cases.GENERAL_VARIANTS:
            got = nat.conv2d(xd, wd, bd, stride=s, padding=p, dilation=d, relu=relu, variant=variant)
            cases.same(_np(got), want, "conv2d %s %s variant %s relu %s" % (case, kind, variant, relu))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.CIN3_CASES)
def test_first_layer(case, kind):
    nat = _nat()
    l = cases.cin3_layer(kind, case)
    xd, wd, bd = _upload(l)
    for relu in RELU:
        cases.same(_np(nat.conv3x3_cin3(xd, wd, bd, relu=relu)), _want(l, relu), "conv3x3_cin3 %s %s relu %s" % (case, kind, relu))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.POOL_CASES)
def test_convolution_with_the_pool_in_its_epilogue(case, kind):
    nat = _nat()
    l = cases.pool_layer(kind, case)
    xd, wd, bd = _upload(l)
    for relu in RELU:
        got = nat.conv2d_same_pool2(xd, wd, bd, dilation=case[6], relu=relu)
        cases.same(_np(got), _want(l, relu, True), "conv2d_same_pool2 %s %s relu %s" % (case, kind, relu))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("has_bias", [False, True])
def test_grouped_launch_of_the_implicit_gemm_kernel(has_bias, kind):
    nat = _nat()
    members = cases.group_layers(kind, cases.GROUP_SHAPES, has_bias, cases.GROUP_1X1)
    ops = [_upload(l) for l in members]
    for relu in RELU:
        got = nat.conv2d_same_group([o[0] for o in ops], [o[1] for o in ops], [o[2] for o in ops] if has_bias else None, relu=relu)
        assert got is not None and len(got) == len(members), "geometry must be supported"
        for i, (l, y) in enumerate(zip(members, got)):
            cases.same(_np(y), _want(l, relu), "conv2d_same_group member %d %s %s relu %s" % (i, l["x"].shape, kind, relu))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("has_bias", [False, True])
def test_grouped_launch_of_the_slab_kernel(has_bias, kind):
    nat = _nat()
    members = cases.group_layers(kind, cases.SLAB_GROUP_SHAPES, has_bias)
    ops = [_upload(l) for l in members]
    for relu in RELU:
        got = nat.conv3x3_halo_group([o[0] for o in ops], [o[1] for o in ops], [o[2] for o in ops] if has_bias else None, relu=relu)
        assert got is not None and len(got) == len(members), "geometry must be supported"
        for i, (l, y) in enumerate(zip(members, got)):
            cases.same(_np(y), _want(l, relu), "conv3x3_halo_group member %d %s %s relu %s" % (i, l["x"].shape, kind, relu))
        # the launch's 80 tile units fit one round of the persistent workgroups; capped at 16 of them every workgroup walks five units, across problems
        got = nat.conv3x3_halo_group([o[0] for o in ops], [o[1] for o in ops], [o[2] for o in ops] if has_bias else None, relu=relu, max_workgroups=16)
        for i, (l, y) in enumerate(zip(members, got)):
            cases.same(_np(y), _want(l, relu), "conv3x3_halo_group on 16 workgroups member %d %s %s relu %s" % (i, l["x"].shape, kind, relu))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.C64_CASES)
def test_resident_filter_kernel_plain_pooled_and_pool_keep(case, kind):
    nat = _nat()
    l = cases.c64_layer(kind, case)
    xd, wd, bd = _upload(l)
    for relu in RELU:
        what = "%s %s relu %s" % (case, kind, relu)
        cases.same(_np(nat.conv3x3_c64(xd, wd, bd, relu=relu, pool=False)), _want(l, relu), "conv3x3_c64 " + what)
        cases.same(_np(nat.conv3x3_c64(xd, wd, bd, relu=relu, pool=True)), _want(l, relu, True), "conv3x3_c64 pool " + what)
        out = nat.conv3x3_c64_pool_keep(xd, wd, bd, relu=relu)
        assert out is not None, "geometry must be supported"
        cases.same(_np(out[0]), _want(l, relu), "conv3x3_c64_pool_keep full " + what)
        cases.same(_np(out[1]), _want(l, relu, True), "conv3x3_c64_pool_keep pooled " + what)


def test_resident_filter_kernel_without_a_bias():
    nat = _nat()
    case = cases.C64_CASES[0]
    for kind in cases.KINDS:
        l = cases.c64_layer(kind, case, False)
        xd, wd, bd = _upload(l)
        assert bd is None
        for relu in RELU:
            cases.same(_np(nat.conv3x3_c64(xd, wd, None, relu=relu, pool=False)), _want(l, relu), "conv3x3_c64 no bias %s relu %s" % (kind, relu))
            cases.same(_np(nat.conv3x3_c64(xd, wd, None, relu=relu, pool=True)), _want(l, relu, True), "conv3x3_c64 no bias pool %s relu %s" % (kind, relu))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.BLOCK_CASES)
def test_fused_first_block(case, kind):
    """conv1_1 (always with its ReLU, its map rounded once) -> conv1_2 [-> pool1]: the chain contract of tests/np_conv_forward.py."""
    nat = _nat()
    ch = cases.block_chain(kind, case)
    l1, l2 = ch["layers"]
    xd, w1, b1, w2, b2 = _nhwc(ch["x"]), _nhwc(l1["w"]), _vec(l1["bias"]), _nhwc(l2["w"]), _vec(l2["bias"])
    assert np.array_equal(_np(xd), ch["x"])
    for relu in RELU:
        for pool in (False, True):
            got = nat.conv1_block(xd, w1, b1, w2, b2, relu=relu, pool=pool)
            cases.same(_np(got), ref.to_bf16(cases.epilogue(ch["maps"][-1], relu, pool)), "conv1_block %s %s relu %s pool %s" % (case, kind, relu, pool))


@pytest.fixture(params=cases.SLAB_MODES)
def slab_mode(request, monkeypatch):
    """SSDHIP_CONVH_MODE (read at every launch): 128 = persistent workgroups prefetching across tiles, pooled calls tile every image;
    1152 = the same with the tolerant waits after an epilogue, pooled calls may tile the stacked batch."""
    monkeypatch.setenv("SSDHIP_CONVH_MODE", request.param)
    return request.param


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case,plans", cases.SLAB_CASES)
def test_slab_kernel_plain_and_pooled(case, plans, kind, slab_mode):
    nat = _nat()
    cases.check_slab_plan(case, False, plans[0])
    cases.check_slab_plan(case, True, plans[1])
    l = cases.slab_layer(kind, case)
    xd, wd, bd = _upload(l)
    for relu in RELU:
        what = "%s %s relu %s mode %s" % (case, kind, relu, slab_mode)
        cases.same(_np(nat.conv3x3_halo(xd, wd, bd, relu=relu, pool=False)), _want(l, relu), "conv3x3_halo " + what)
        cases.same(_np(nat.conv2d_same(xd, wd, bd, dilation=1, relu=relu, variant=7)), _want(l, relu), "conv2d_same variant 7 " + what)
        cases.same(_np(nat.conv3x3_halo(xd, wd, bd, relu=relu, pool=True)), _want(l, relu, True), "conv3x3_halo pool " + what)


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case,plan", cases.SLAB_POOL_CASES)
def test_slab_kernel_pooled_on_the_stacked_batch_and_small_maps(case, plan, kind, slab_mode):
    nat = _nat()
    cases.check_slab_plan(case, True, plan)
    l = cases.slab_layer(kind, case)
    xd, wd, bd = _upload(l)
    for relu in RELU:
        got = nat.conv3x3_halo(xd, wd, bd, relu=relu, pool=True)
        cases.same(_np(got), _want(l, relu, True), "conv3x3_halo pool %s %s relu %s mode %s" % (case, kind, relu, slab_mode))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", [c for c, _ in cases.SLAB_CASES + cases.SLAB_POOL_CASES])
def test_slab_kernel_pool_keep_writes_both_maps(case, kind, monkeypatch):
    nat = _nat()
    monkeypatch.delenv("SSDHIP_CONVH_MODE", raising=False)
    l = cases.slab_layer(kind, case)
    xd, wd, bd = _upload(l)
    for relu in RELU:
        out = nat.conv3x3_halo_pool_keep(xd, wd, bd, relu=relu)
        assert out is not None, "geometry must be supported"
        cases.same(_np(out[0]), _want(l, relu), "conv3x3_halo_pool_keep full %s %s relu %s" % (case, kind, relu))
        cases.same(_np(out[1]), _want(l, relu, True), "conv3x3_halo_pool_keep pooled %s %s relu %s" % (case, kind, relu))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.SLAB_STRIDED_CASES)
def test_slab_kernel_strided_and_cropped(case, kind):
    nat = _nat()
    l = cases.slab_strided_layer(kind, case)
    xd, wd, bd = _upload(l)
    for relu in RELU:
        got = nat.conv2d(xd, wd, bd, stride=case[5], padding=case[6], relu=relu, variant=7)
        cases.same(_np(got), _want(l, relu), "conv2d variant 7 %s %s relu %s" % (case, kind, relu))


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.IMAGE_CASES)
def test_image_resident_kernel(case, kind, monkeypatch):
    nat = _nat()
    b, h, w, cin, cout, k, s, p, d = case
    l = cases.image_layer(kind, case)
    xd, wd, bd = _upload(l)
    assert nat.conv2d_image_supported(xd, wd, s, p, d), "geometry must be supported"
    for relu in RELU:
        what = "%s %s relu %s" % (case, kind, relu)
        want = _want(l, relu)
        cases.same(_np(nat.conv2d_image(xd, wd, bd, stride=s, padding=p, dilation=d, relu=relu)), want, "conv2d_image " + what)
        if k == 3 and s == 1 and p == d:
            assert nat.conv3x3_image_supported(xd, wd, d), "geometry must be supported"
            cases.same(_np(nat.conv3x3_image(xd, wd, bd, dilation=d, relu=relu)), want, "conv3x3_image " + what)
        if k == 1:                                            # the other tiling of a 1 x 1 layer: whole-image tiles
            monkeypatch.setenv("SSDHIP_CONVIMG_PXT", "0")
            cases.same(_np(nat.conv2d_image(xd, wd, bd, stride=s, padding=p, dilation=d, relu=relu)), want, "conv2d_image whole-image tiles " + what)
            monkeypatch.delenv("SSDHIP_CONVIMG_PXT")


@pytest.mark.parametrize("kind", cases.KINDS)
@pytest.mark.parametrize("case", cases.CHAIN_CASES)
def test_chain_kernel_every_kept_map(case, kind):
    nat = _nat()
    spec = case[4]
    ch = cases.chain_chain(kind, case)
    xd = _nhwc(ch["x"])
    assert np.array_equal(_np(xd), ch["x"])
    packed = [nat.conv_chain_pack(_nhwc(l["w"])) for l in ch["layers"]]
    assert all(pk is not None for pk in packed), "geometry must be supported"
    for relu in RELU:                                         # the LAST layer without and with its ReLU; the others as the case says
        layers = []
        for i, ((k, s, p, cout, r, keep), l, pk) in enumerate(zip(spec, ch["layers"], packed)):
            last = i == len(spec) - 1
            layers.append(dict(packed=pk, bias=_vec(l["bias"]), k=k, stride=s, pad=p, cout=cout, relu=int(relu if last else r), keep=bool(keep)))
        got = nat.conv_chain(xd, layers)
        kept = [i for i, sp in enumerate(spec) if sp[5]]
        assert got is not None and len(got) == len(kept), "geometry must be supported"
        for y, i in zip(got, kept):
            exact = cases.epilogue(ch["maps"][i], relu) if i == len(spec) - 1 else ch["maps"][i]
            cases.same(_np(y), ref.to_bf16(exact), "conv_chain %s %s layer %d last relu %s" % (case[:4], kind, i, relu))
