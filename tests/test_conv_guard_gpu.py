"""What tests/test_forward_exact_gpu.py cannot see of the inference convolution kernels (csrc/ssdhip_conv.hip, ssdhip_conv64.hip,
ssdhip_convh.hip, ssdhip_convimg.hip, ssdhip_chain.hip), on the same entries, modes and case tables (tests/forward_exact_cases.py, "unit"
data: addressing does not depend on the data kind), through the guard bands of tests/guarded.py:

  A. every output element is written: outputs are allocated full of 0xFF bytes (NaN) and must equal the float64 reference rounded once;
  B. nothing outside an output is written: the bands around every map `_native._empty_nhwc` hands out (and around the operands) keep
     their fill;
  C. nothing outside an operand influences a result: x, the filters and the bias sit between bands of 0x00, 0xFF (NaN) and 0x7F7F (the
     largest finite bf16) in turn, and the three results are bit-identical (the split-K workspace is filled with 0xFF before the call);
  D. non-finite values stay where the convolution puts them: one image all NaN (the first, the last, a middle one) leaves every other
     image's output bit-identical, under every epilogue; one member all NaN leaves the other members of a grouped launch alone; one
     NaN element of x makes NaN exactly the outputs with a tap on it (guarded.receptive_mask: tap arithmetic, no second convolution)
     in all channels, and changes no other bit -- single layers without ReLU and pool only.

Every access these tests can provoke lands inside a buffer the test owns: the bands are at least 1 MiB and at least four times the
largest displacement a kernel adds to a descriptor base (guarded.band_bytes).  What they cannot show: a load that lands in a band and is
then DISCARDED by a select changes no result and is not seen; nor is a load further out than a band.  What ReLU or pooling make of a NaN
inside its own window is not specified here.  No tolerance, no cap on differing elements; an entry that returns None for a table case
fails.  Needs an MI355X."""
import numpy as np
import pytest

from tests import forward_exact_cases as cases
from tests import guarded
from tests import np_conv_forward as ref

pytestmark = pytest.mark.gpu

RELU = (False, True)
KIND = "unit"


def _nat():
    from ssd_keras_amd import _native as nat
    return nat


def _dev(a):
    """A float64 array of bf16 values -> bf16 CUDA tensor, same shape."""
    import torch
    return torch.from_numpy(np.array(a, dtype=np.float64)).to(torch.bfloat16).cuda()


def _band(x_shape, dilation=1, channels=0):
    return guarded.band_bytes(dilation, x_shape[2], max(x_shape[3], channels))


def _layer_ops(l, band, passes_nhwc=True):
    """{fill: Operands} of one layer of cases.layer(): arg = (x, w, bias).  passes_nhwc: the entry sends x through _nhwc_bf16 (the
    3-channel entries check the layout themselves)."""
    xh, wh, bh = _dev(l["x"]), _dev(l["w"]), None if l["bias"] is None else _dev(l["bias"])
    out = {}
    for fill in guarded.FILLS:
        x, w = guarded.banded(xh, fill, band, nhwc=True), guarded.banded(wh, fill, band, nhwc=True)
        bias = None if bh is None else guarded.banded(bh, fill, band)
        assert x.permute(0, 2, 3, 1).is_contiguous()
        out[fill] = guarded.Operands(fill, (x, w, bias), [x], [w, bias], ([x] if passes_nhwc else []) + [w])
    return out


def _group_ops(members, band, has_bias):
    """{fill: Operands} of a grouped launch: arg = (xs, ws, biases or None)."""
    host = [(_dev(l["x"]), _dev(l["w"]), _dev(l["bias"]) if has_bias and l["bias"] is not None else None) for l in members]
    out = {}
    for fill in guarded.FILLS:
        xs = [guarded.banded(h[0], fill, band, nhwc=True) for h in host]
        ws = [guarded.banded(h[1], fill, band, nhwc=True) for h in host]
        bs = [None if h[2] is None else guarded.banded(h[2], fill, band) for h in host]
        out[fill] = guarded.Operands(fill, (xs, ws, bs if has_bias else None), xs, ws + bs, xs + ws)
    return out


class _Wants:
    """The exact maps of a case on the device, (B, C, H, W) views, built once per (relu, pool)."""

    def __init__(self, exact):
        self.exact, self.made = exact, {}

    def __call__(self, *key):
        if key not in self.made:
            self.made[key] = [_dev(ref.to_bf16(a)).permute(0, 3, 1, 2) for a in self.exact(*key)]
        return self.made[key]


def _check(monkeypatch, what, ops, call, wants, band, geometry=None, which=0, isolate="image"):
    """A, B, C of one call form; then D on the operands between 0x00 bands: `isolate` = "image" (where B >= 2) or "member";
    `geometry` = (k, stride, pad, dilation) of a single layer run without ReLU and pool: element locality on result `which`."""
    nat = _nat()
    clean = guarded.check_written_confined_deaf(monkeypatch, nat, ops, call, wants, band, what)
    base = ops[guarded.FILLS[0]]
    if isolate == "member":
        guarded.check_member_isolation(monkeypatch, nat, base, call, clean, band, what)
    if base.maps[0].shape[0] >= 2:
        guarded.check_image_isolation(monkeypatch, nat, base, call, clean, band, what)
    if geometry is not None:
        guarded.check_element_locality(monkeypatch, nat, base, call, clean, geometry, band, what, which)


@pytest.mark.parametrize("case", cases.SAME_CASES)
def test_same_convolution_every_variant(case, monkeypatch):
    nat = _nat()
    k, d = case[5], case[6]
    l = cases.same_layer(KIND, case)
    band = _band(l["x"].shape, d)
    ops, wants = _layer_ops(l, band), _Wants(lambda relu: [cases.epilogue(l["pre"], relu)])
    for relu in RELU:
        for variant in cases.SAME_VARIANTS:
            _check(monkeypatch, "conv2d_same %s variant %s relu %s" % (case, variant, relu), ops,
                   lambda a: [nat.conv2d_same(*a, dilation=d, relu=relu, variant=variant)], wants(relu), band,
                   None if relu else (k, 1, d * (k // 2), d))


@pytest.mark.parametrize("case,plan", cases.GENERAL_CASES)
def test_general_convolution_every_variant_and_split_k(case, plan, monkeypatch):
    import torch
    nat = _nat()
    b, h, w, cin, cout, k, s, p, d, _ = case
    l = cases.general_layer(KIND, case)
    band = _band(l["x"].shape, d)
    ops, wants = _layer_ops(l, band), _Wants(lambda relu: [cases.epilogue(l["pre"], relu)])
    need = nat.load().ssdhip_conv2d_splitk_workspace_bytes(b, h, w, cin, cout, k, s, p, d, 0)
    assert need > 0, "geometry must be supported"

    def call(a, relu, variant):
        if variant == 8:                                      # partial tiles a range did not write must not reach the reduction
            nat.workspaces.get(torch.device("cuda", torch.cuda.current_device()), "conv_splitk", need).fill_(0xFF)
        return [nat.conv2d(*a, stride=s, padding=p, dilation=d, relu=relu, variant=variant)]

    for relu in RELU:
        for variant in cases.GENERAL_VARIANTS:
            _check(monkeypatch, "conv2d %s variant %s relu %s" % (case, variant, relu), ops, lambda a: call(a, relu, variant), wants(relu), band,
                   None if relu else (k, s, p, d))


@pytest.mark.parametrize("case", cases.CIN3_CASES)
def test_first_layer(case, monkeypatch):
    nat = _nat()
    l = cases.cin3_layer(KIND, case)
    band = _band(l["x"].shape, 1, 64)
    ops, wants = _layer_ops(l, band, passes_nhwc=False), _Wants(lambda relu: [cases.epilogue(l["pre"], relu)])
    for relu in RELU:
        _check(monkeypatch, "conv3x3_cin3 %s relu %s" % (case, relu), ops, lambda a: [nat.conv3x3_cin3(*a, relu=relu)], wants(relu), band,
               None if relu else (3, 1, 1, 1))


@pytest.mark.parametrize("case", cases.POOL_CASES)
def test_convolution_with_the_pool_in_its_epilogue(case, monkeypatch):
    nat = _nat()
    d = case[6]
    l = cases.pool_layer(KIND, case)
    band = _band(l["x"].shape, d)
    ops, wants = _layer_ops(l, band), _Wants(lambda relu: [cases.epilogue(l["pre"], relu, True)])
    for relu in RELU:
        _check(monkeypatch, "conv2d_same_pool2 %s relu %s" % (case, relu), ops, lambda a: [nat.conv2d_same_pool2(*a, dilation=d, relu=relu)],
               wants(relu), band)


def _group_geometries(members):
    return [(l["w"].shape[1],) + l["geometry"] for l in members]


def _check_group(monkeypatch, what, members, ops, call, wants, band, relu):
    """A grouped launch: A, B, C, whole members and whole images NaN; element locality member by member (each a single layer)."""
    nat = _nat()
    _check(monkeypatch, what, ops, call, wants, band, isolate="member")
    if relu:
        return
    base = ops[guarded.FILLS[0]]
    clean = guarded.guarded_call(monkeypatch, nat, call, base, band, what)
    for i, geometry in enumerate(_group_geometries(members)):
        one = guarded.Operands(base.fill_byte, base.arg, [base.maps[i]], [], [])
        guarded.check_element_locality(monkeypatch, nat, one, call, clean, geometry, band, "%s member %d" % (what, i), i, True)


@pytest.mark.parametrize("has_bias", [False, True])
def test_grouped_launch_of_the_implicit_gemm_kernel(has_bias, monkeypatch):
    nat = _nat()
    members = cases.group_layers(KIND, cases.GROUP_SHAPES, has_bias, cases.GROUP_1X1)
    band = max(_band(l["x"].shape) for l in members)
    ops, wants = _group_ops(members, band, has_bias), _Wants(lambda relu: [cases.epilogue(l["pre"], relu) for l in members])
    for relu in RELU:
        _check_group(monkeypatch, "conv2d_same_group bias %s relu %s" % (has_bias, relu), members, ops,
                     lambda a: nat.conv2d_same_group(*a, relu=relu), wants(relu), band, relu)


@pytest.mark.parametrize("max_workgroups", [0, 16])
@pytest.mark.parametrize("has_bias", [False, True])
def test_grouped_launch_of_the_slab_kernel(has_bias, max_workgroups, monkeypatch):
    """max_workgroups=16: every persistent workgroup walks five tile units, across problems."""
    nat = _nat()
    members = cases.group_layers(KIND, cases.SLAB_GROUP_SHAPES, has_bias)
    band = max(_band(l["x"].shape) for l in members)
    ops, wants = _group_ops(members, band, has_bias), _Wants(lambda relu: [cases.epilogue(l["pre"], relu) for l in members])
    for relu in RELU:
        _check_group(monkeypatch, "conv3x3_halo_group bias %s on %d workgroups relu %s" % (has_bias, max_workgroups, relu), members, ops,
                     lambda a: nat.conv3x3_halo_group(*a, relu=relu, max_workgroups=max_workgroups), wants(relu), band, relu)


def _full_and_pooled(l):
    return _Wants(lambda relu, pool: [cases.epilogue(l["pre"], relu, q) for q in ((False, True) if pool == "keep" else (pool,))])


def _check_c64(monkeypatch, case, l, what):
    nat = _nat()
    band = _band(l["x"].shape)
    ops, wants = _layer_ops(l, band), _full_and_pooled(l)
    for relu in RELU:
        tail = "%s %s relu %s" % (what, case, relu)
        local = None if relu else (3, 1, 1, 1)
        _check(monkeypatch, "conv3x3_c64 " + tail, ops, lambda a: [nat.conv3x3_c64(*a, relu=relu, pool=False)], wants(relu, False), band, local)
        _check(monkeypatch, "conv3x3_c64 pool " + tail, ops, lambda a: [nat.conv3x3_c64(*a, relu=relu, pool=True)], wants(relu, True), band)
        if l["bias"] is not None:
            _check(monkeypatch, "conv3x3_c64_pool_keep " + tail, ops, lambda a: nat.conv3x3_c64_pool_keep(*a, relu=relu), wants(relu, "keep"),
                   band, local)


@pytest.mark.parametrize("case", cases.C64_CASES)
def test_resident_filter_kernel_plain_pooled_and_pool_keep(case, monkeypatch):
    _check_c64(monkeypatch, case, cases.c64_layer(KIND, case), "")


def test_resident_filter_kernel_without_a_bias(monkeypatch):
    case = cases.C64_CASES[0]
    _check_c64(monkeypatch, case, cases.c64_layer(KIND, case, False), "no bias")


@pytest.mark.parametrize("case", cases.BLOCK_CASES)
def test_fused_first_block(case, monkeypatch):
    nat = _nat()
    ch = cases.block_chain(KIND, case)
    l1, l2 = ch["layers"]
    band = _band(ch["x"].shape, 1, 64)
    host = [_dev(a) for a in (ch["x"], l1["w"], l1["bias"], l2["w"], l2["bias"])]
    ops = {}
    for fill in guarded.FILLS:
        x, w1, w2 = (guarded.banded(host[i], fill, band, nhwc=True) for i in (0, 1, 3))
        b1, b2 = (guarded.banded(host[i], fill, band) for i in (2, 4))
        assert x.permute(0, 2, 3, 1).is_contiguous()
        ops[fill] = guarded.Operands(fill, (x, w1, b1, w2, b2), [x], [w1, b1, w2, b2], [w1, w2])
    wants = _Wants(lambda relu, pool: [cases.epilogue(ch["maps"][-1], relu, pool)])
    for relu in RELU:
        for pool in (False, True):
            _check(monkeypatch, "conv1_block %s relu %s pool %s" % (case, relu, pool), ops, lambda a: [nat.conv1_block(*a, relu=relu, pool=pool)],
                   wants(relu, pool), band)


@pytest.fixture(params=cases.SLAB_MODES)
def slab_mode(request, monkeypatch):
    """SSDHIP_CONVH_MODE, as in tests/test_forward_exact_gpu.py."""
    monkeypatch.setenv("SSDHIP_CONVH_MODE", request.param)
    return request.param


@pytest.mark.parametrize("case,plans", cases.SLAB_CASES)
def test_slab_kernel_plain_and_pooled(case, plans, slab_mode, monkeypatch):
    nat = _nat()
    cases.check_slab_plan(case, False, plans[0])
    cases.check_slab_plan(case, True, plans[1])
    l = cases.slab_layer(KIND, case)
    band = _band(l["x"].shape)
    ops, wants = _layer_ops(l, band), _full_and_pooled(l)
    for relu in RELU:
        tail = "%s relu %s mode %s" % (case, relu, slab_mode)
        local = None if relu else (3, 1, 1, 1)
        _check(monkeypatch, "conv3x3_halo " + tail, ops, lambda a: [nat.conv3x3_halo(*a, relu=relu, pool=False)], wants(relu, False), band, local)
        _check(monkeypatch, "conv2d_same variant 7 " + tail, ops, lambda a: [nat.conv2d_same(*a, dilation=1, relu=relu, variant=7)],
               wants(relu, False), band, local)
        _check(monkeypatch, "conv3x3_halo pool " + tail, ops, lambda a: [nat.conv3x3_halo(*a, relu=relu, pool=True)], wants(relu, True), band)


@pytest.mark.parametrize("case,plan", cases.SLAB_POOL_CASES)
def test_slab_kernel_pooled_on_the_stacked_batch_and_small_maps(case, plan, slab_mode, monkeypatch):
    nat = _nat()
    cases.check_slab_plan(case, True, plan)
    l = cases.slab_layer(KIND, case)
    band = _band(l["x"].shape)
    ops, wants = _layer_ops(l, band), _full_and_pooled(l)
    for relu in RELU:
        _check(monkeypatch, "conv3x3_halo pool %s relu %s mode %s" % (case, relu, slab_mode), ops,
               lambda a: [nat.conv3x3_halo(*a, relu=relu, pool=True)], wants(relu, True), band)


@pytest.mark.parametrize("case", [c for c, _ in cases.SLAB_CASES + cases.SLAB_POOL_CASES])
def test_slab_kernel_pool_keep_writes_both_maps(case, monkeypatch):
    nat = _nat()
    monkeypatch.delenv("SSDHIP_CONVH_MODE", raising=False)
    l = cases.slab_layer(KIND, case)
    band = _band(l["x"].shape)
    ops, wants = _layer_ops(l, band), _full_and_pooled(l)
    for relu in RELU:
        _check(monkeypatch, "conv3x3_halo_pool_keep %s relu %s" % (case, relu), ops, lambda a: nat.conv3x3_halo_pool_keep(*a, relu=relu),
               wants(relu, "keep"), band, None if relu else (3, 1, 1, 1))


@pytest.mark.parametrize("case", cases.SLAB_STRIDED_CASES)
def test_slab_kernel_strided_and_cropped(case, monkeypatch):
    nat = _nat()
    s, p = case[5], case[6]
    l = cases.slab_strided_layer(KIND, case)
    band = _band(l["x"].shape)
    ops, wants = _layer_ops(l, band), _Wants(lambda relu: [cases.epilogue(l["pre"], relu)])
    for relu in RELU:
        _check(monkeypatch, "conv2d variant 7 %s relu %s" % (case, relu), ops,
               lambda a: [nat.conv2d(*a, stride=s, padding=p, relu=relu, variant=7)], wants(relu), band, None if relu else (3, s, p, 1))


@pytest.mark.parametrize("case", cases.IMAGE_CASES)
def test_image_resident_kernel(case, monkeypatch):
    nat = _nat()
    b, h, w, cin, cout, k, s, p, d = case
    l = cases.image_layer(KIND, case)
    band = _band(l["x"].shape, d)
    ops, wants = _layer_ops(l, band), _Wants(lambda relu: [cases.epilogue(l["pre"], relu)])
    x0, w0, _ = ops[guarded.FILLS[0]].arg
    assert nat.conv2d_image_supported(x0, w0, s, p, d), "geometry must be supported"
    for relu in RELU:
        tail = "%s relu %s" % (case, relu)
        local = None if relu else (k, s, p, d)
        general = lambda a: [nat.conv2d_image(*a, stride=s, padding=p, dilation=d, relu=relu)]
        _check(monkeypatch, "conv2d_image " + tail, ops, general, wants(relu), band, local)
        if k == 3 and s == 1 and p == d:
            assert nat.conv3x3_image_supported(x0, w0, d), "geometry must be supported"
            _check(monkeypatch, "conv3x3_image " + tail, ops, lambda a: [nat.conv3x3_image(*a, dilation=d, relu=relu)], wants(relu), band, local)
        if k == 1:                                            # the other tiling of a 1 x 1 layer: whole-image tiles
            monkeypatch.setenv("SSDHIP_CONVIMG_PXT", "0")
            _check(monkeypatch, "conv2d_image whole-image tiles " + tail, ops, general, wants(relu), band, local)
            monkeypatch.delenv("SSDHIP_CONVIMG_PXT")


@pytest.mark.parametrize("case", cases.CHAIN_CASES)
def test_chain_kernel_every_kept_map(case, monkeypatch):
    """The packed filters are the kernel's operand: they are packed INTO a banded buffer.  Image isolation only (a chain of layers)."""
    import torch
    nat = _nat()
    spec = case[4]
    ch = cases.chain_chain(KIND, case)
    band = _band(ch["x"].shape, 1, max(sp[3] for sp in spec))
    xh, whs, bhs = _dev(ch["x"]), [_dev(l["w"]).permute(0, 3, 1, 2) for l in ch["layers"]], [_dev(l["bias"]) for l in ch["layers"]]
    sizes = [nat.conv_chain_pack(wh) for wh in whs]
    assert all(pk is not None for pk in sizes), "geometry must be supported"
    ops = {}
    for fill in guarded.FILLS:
        x = guarded.banded(xh, fill, band, nhwc=True)
        packed = [nat.conv_chain_pack(wh, out=guarded.banded(torch.zeros_like(pk), fill, band)) for wh, pk in zip(whs, sizes)]
        biases = [guarded.banded(bh, fill, band) for bh in bhs]
        ops[fill] = guarded.Operands(fill, (x, packed, biases), [x], packed + biases, [x])
    kept = [i for i, sp in enumerate(spec) if sp[5]]
    last = len(spec) - 1
    wants = _Wants(lambda relu: [cases.epilogue(ch["maps"][i], relu) if i == last else ch["maps"][i] for i in kept])

    def call(a, relu):                                        # the LAST layer without and with its ReLU; the others as the case says
        x, packed, biases = a
        return nat.conv_chain(x, [dict(packed=pk, bias=bias, k=k, stride=s, pad=p, cout=cout, relu=int(relu if i == last else r), keep=bool(keep))
                                  for i, ((k, s, p, cout, r, keep), pk, bias) in enumerate(zip(spec, packed, biases))])

    for relu in RELU:
        _check(monkeypatch, "conv_chain %s last relu %s" % (case[:4], relu), ops, lambda a: call(a, relu), wants(relu), band)
