"""Which libssdhip kernels can run a convolution layer: ONE description for the inference path, its pooled form and both halves of the
training step (`SSDModel.conv_act` / `conv_act_pool` / `conv1_block_pool` / `_train_thunk`, the autograd nodes of `_train_fns`).

A layer is a `Geometry` (plain ints), the kernels' limits are predicates of it, and `candidates` lists, in the order the autotune
(`SSDModel._pick`) times them, every form offered to a context as `name -> (x, w, b) -> y`.  What differs between the contexts is data
in that list ("igemm5 and splitk: inference only"), not a second copy of it.  The backward pass times nothing: `dgrad` and `WGRAD_FORMS`
name its kernels in the order tried, the predicates below them say where the step's fused forms apply, and `_train_fns` maps the names to
`_native` calls.  `switch` / `on` read the SSDHIP_* switches of the models package from os.environ at call time: no cache.
"""
import os
from collections import namedtuple

from .. import _native as nat

# every SSDHIP_* switch the models package reads, with its default (None: unset).  "NO_*" and the other "1"-switches are tested with `on`.
SWITCHES = {
    "CONV": "auto", "PREFER": None, "GEMM_1X1": "0", "IMAGE2": "1",
    "NO_HALO": "0", "NO_IMAGE": "0", "NO_SPLITK": "0", "NO_CONV1_BLOCK": "0", "NO_CHAIN": "0", "NO_POOL_NORM": "0",
    "NO_HALO_MIXED": "0", "HEAD_OVERLAP": None, "GRAPH_HEAD_OVERLAP": "4", "HEAD_SPLIT": "3", "HEAD_WGS": None, "SIDE_PRIORITY": "0",
    "NO_OWN_DGRAD": "0", "NO_OWN_WGRAD": "0", "NO_TAPS_BWD": "0", "NO_MASKED_DGRAD": "0", "NO_MASKED_SUMS": "0", "NO_C64_DGRAD": "0",
    "NO_CONV1_1_BWD": "0", "NO_POOL_KEEP": "0", "NO_HALO_POOL_KEEP": "0", "NO_FUSED_POOL_BWD": "0", "NO_OWN_POOL": "0",
    "NO_TRAIN_PREPROCESS": "0", "NO_TRAIN_ASSEMBLY": "0", "NO_OWN_HEADS": "0",
}


def switch(name):
    """The value of SSDHIP_<name>, or its default."""
    return os.environ.get("SSDHIP_" + name, SWITCHES[name])


def on(name):
    return switch(name) == "1"


def autotuned():
    """SSDHIP_CONV leaves the choice to the autotune and SSDHIP_PREFER names no form: what every untimed shortcut asks first."""
    return switch("CONV") in ("auto", "auto_miopen") and not switch("PREFER")


Geometry = namedtuple("Geometry", "batch h w cin cout k stride padding dilation groups bias")
_Shape = namedtuple("_Shape", "shape")                   # what nat.conv2d_image_supported reads of a tensor


def _square(kh, kw, stride, padding, dilation):
    return (kh == kw and isinstance(padding, tuple) and stride[0] == stride[1] and padding[0] == padding[1] and dilation[0] == dilation[1])


def geometry_of(conv, x=None):
    """The layer `conv` [applied to the (B, Cin, H, W) map x]; None for what no kernel here covers anyway: a non-square filter, stride,
    padding or dilation, padding given as a string or a padding mode other than zeros."""
    if not _square(*conv.kernel_size, conv.stride, conv.padding, conv.dilation) or conv.padding_mode != 'zeros':
        return None
    b, _, h, w = x.shape if x is not None else (0, 0, 0, 0)
    return Geometry(b, h, w, conv.in_channels, conv.out_channels, conv.kernel_size[0], conv.stride[0],
                    conv.padding[0], conv.dilation[0], conv.groups, int(conv.bias is not None))


def geometry_of_grads(wb, xb, stride, padding, dilation):
    """The same record in the backward pass, from the saved (Cout, Cin, k, k) filters and the layer's input."""
    if not _square(wb.shape[2], wb.shape[3], stride, tuple(padding), dilation):
        return None
    return Geometry(xb.shape[0], xb.shape[2], xb.shape[3], wb.shape[1], wb.shape[0], wb.shape[2], stride[0], padding[0], dilation[0], 1, 1)


def out_side(n, g):
    return (n + 2 * g.padding - g.dilation * (g.k - 1) - 1) // g.stride + 1


# -- the kernels' limits -------------------------------------------------------------------------------------------------------------
def first_layer(g):
    """csrc/ssdhip_conv.hip, conv3x3_cin3: the 3 -> 64 channel 3x3 'same' layer on the image."""
    return g is not None and g[3:] == (3, 64, 3, 1, 1, 1, 1, 1)


def igemm(g):
    """csrc/ssdhip_conv.hip, nat.conv2d_same: stride-1 'same' 1x1 / 3x3 layers (any dilation), channel counts multiples of 64."""
    return (g is not None and g.k in (1, 3) and g.stride == 1 and g.groups == 1 and g.padding == g.dilation * (g.k // 2)
            and g.cin % 64 == 0 and g.cout % 64 == 0 and bool(g.bias))


def igemm_general(g):
    """Strided / partially padded 3x3 and 1x1 layers (conv6_2 ... conv9_2) for nat.conv2d."""
    return (g is not None and g.k in (1, 3) and 1 <= g.stride <= 4 and g.groups == 1 and 0 <= g.padding <= g.dilation * (g.k // 2)
            and g.cin % 64 == 0 and g.cout % 64 == 0 and bool(g.bias))


def few_tiles(m_pixels, cout):
    """Fewer 128 x 128 output tiles than a third of the CUs: the layer's one-pass kernels leave most of the chip idle while a few
    workgroups walk their whole K loop (the SSD extra layers behind fc7)."""
    return -(-m_pixels // 128) * -(-cout // 128) <= 100


def splitk_measured_regime(g):
    """Where the split-K form was measured inside the graphed step (profiles/r03p_*: the SSD300 / SSD512 extra layers behind fc7 at
    batch 32: maps of at most 19 x 19 ... 32 x 32 pixels, a batch that fills the K ranges): only there is it taken without a timing
    run.  Everywhere else (small batches, where `few_tiles` also covers conv3_x ... fc7) it is an ordinary autotune candidate."""
    return g.batch >= 16 and g.h * g.w <= 32 * 32


def halo(g):
    """csrc/ssdhip_convh.hip: 3x3, dilation 1, Cin and Cout multiples of 128 (maps up to 94 wide on the padded position grid,
    wider ones and the pooled form on 2-D tiles)."""
    return g.k == 3 and g.dilation == 1 and g.cin % 128 == 0 and g.cout % 128 == 0 and not on("NO_HALO")


def halo_strided(g):
    """The slab kernel keeps the strided / cropped positions of the stride-1 'same' result: redundant FLOPs, but the extra layers cost
    the latency of their K loop, not arithmetic."""
    return (halo(g) and g.stride in (1, 2) and g.padding in (0, 1) and g.w <= 94 and g.h + 2 * g.padding >= 3 and g.w + 2 * g.padding >= 3)


def c64(g):
    """csrc/ssdhip_conv64.hip: the resident-filter kernel of the 3x3 layers with 64 input channels."""
    return g.cin == 64 and g.k == 3 and g.dilation == 1


def _half_a_chip(g):
    return g.batch * (g.cout // 64) >= 128


def image(g):
    """csrc/ssdhip_convimg.hip: 3x3 'same' with any dilation, the whole map of an image (at most 384 pixels) resident in LDS, one
    tile per (image, 128 output channels) -- offered where that gives at least half a chip's worth of tiles."""
    return (g.k == 3 and g.h * g.w <= 384 and g.cin % 64 == 0 and g.cout % 64 == 0 and 1 <= g.dilation <= 16 and _half_a_chip(g)
            and not on("NO_IMAGE"))


def image2(g):
    """Round 6, csrc/ssdhip_convimg.hip's general form: 1 x 1 layers (fc7, conv6_1: one step per 64-channel slice of the resident
    image) and strided / partially padded 3 x 3 layers (conv6_2) on maps of at most 384 pixels, where one image x 64 output channels
    per tile gives at least half a chip's worth of tiles."""
    if switch("IMAGE2") == "0" or on("NO_IMAGE") or g.groups != 1:
        return False
    return _half_a_chip(g) and nat.conv2d_image_supported(_Shape((g.batch, g.cin, g.h, g.w)), _Shape((g.cout, g.cin, g.k, g.k)), g.stride,
                                                          g.padding, g.dilation)


def own_dgrad(g):
    """The data gradient of this layer runs on libssdhip's forward kernels with transposed / flipped filters (see `dgrad`): k in (1, 3),
    channel counts multiples of 64; stride 1 and 'same', or (round 6) a strided / 'valid' 3 x 3 layer behind an embedding launch."""
    return g is not None and g.groups == 1 and (dgrad_same(g) or dgrad_embedded(g))


def dgrad_same(g):
    return g.stride == 1 and g.k in (1, 3) and g.padding == g.dilation * (g.k // 2) and g.cin % 64 == 0 and g.cout % 64 == 0


def dgrad_embedded(g):
    """(round 6) a strided or 'valid' 3 x 3 layer (conv6_2 / conv7_2: stride 2 behind ZeroPadding2D; conv8_2 / conv9_2: no padding):
    dX[r] = sum_k dY[(r + pad - k) / s] w[k] is the 3 x 3 'same' convolution of Z -- zeros with dY at (1 - pad + s i) -- with the same
    transposed, tap-flipped filters: one embedding launch (csrc/ssdhip_train.hip), then the data gradient of a 'same' layer."""
    return (not dgrad_same(g) and g.k == 3 and g.dilation == 1 and g.padding in (0, 1) and g.cin % 64 == 0 and g.cout % 64 == 0)


def dgrad_geometry(g):
    """The data gradient of a layer as a layer of its own: the stride-1 'same' convolution of dL/dy (embedded where the layer is strided
    or 'valid') with the filters transposed (Cin <-> Cout) and their taps flipped, no bias."""
    return g._replace(cin=g.cout, cout=g.cin, stride=1, padding=g.dilation * (g.k // 2))


# -- the candidates ------------------------------------------------------------------------------------------------------------------
INFERENCE, POOLED, TRAINING, DGRAD = "inference", "pooled", "training", "dgrad"
_EVERYWHERE = (INFERENCE, POOLED, TRAINING, DGRAD)
_UNPOOLED = (INFERENCE, TRAINING, DGRAD)
DGRAD_PRIORITY = ("image", "halo", "c64", "igemm")       # no timing run in the backward pass: the most specific form offered
UNTIMED_PRIORITY = ("image", "splitk")


def _forms(g, relu, context):
    """(name, contexts that are offered it, the geometry qualifies, taken without a timing run where `untimed_choice` allows, launch)
    in the order of the autotune."""
    if igemm(g):
        d, p = g.dilation, g.padding
        pixels = g.batch * g.h * g.w
        return (
            ("igemm", _EVERYWHERE, True, False, lambda x, w, b: nat.conv2d_same(x, w, b, dilation=d, relu=relu)),
            # the three-stage / 32-channel-slice / 3-workgroups-per-CU variant wins on the shallow-K layers (Cin = 64)
            ("igemm6", (INFERENCE, POOLED, TRAINING), True, False, lambda x, w, b: nat.conv2d_same(x, w, b, dilation=d, relu=relu, variant=6)),
            # at most one workgroup per CU: the deepest ring too
            ("igemm5", (INFERENCE,), pixels <= 128 * 128, False, lambda x, w, b: nat.conv2d_same(x, w, b, dilation=d, relu=relu, variant=5)),
            # the split-K form: the K ranges of a tile side by side on otherwise idle CUs
            ("splitk", (INFERENCE,), few_tiles(pixels, g.cout), splitk_measured_regime(g) and not on("NO_SPLITK"),
             lambda x, w, b: nat.conv2d(x, w, b, stride=1, padding=p, dilation=d, relu=relu, variant=8)),
            # (data gradient: a 64-channel dL/dy -- conv1_2 -- the same bits as the implicit-GEMM kernel in half its time, 430 -> 215 us
            #  at 300 x 300 / batch 32)
            ("c64", _UNPOOLED, c64(g) and not (context == DGRAD and on("NO_C64_DGRAD")), False,
             lambda x, w, b: nat.conv3x3_c64(x, w, b, relu=relu, pool=False)),
            # (bit-identical to the implicit-GEMM kernel and faster on the deep 3x3 layers, r02o)
            ("halo", _EVERYWHERE, halo(g), False, lambda x, w, b: nat.conv2d_same(x, w, b, dilation=1, relu=relu, variant=7)),
            # one image per tile, the dilated taps as per-lane LDS addresses: fc6, conv5_x
            ("image", _EVERYWHERE, image(g), False, lambda x, w, b: nat.conv3x3_image(x, w, b, dilation=d, relu=relu)),
            # round 6: a 1 x 1 layer with the image's 64-channel slices resident in LDS, one step per slice (fc7 41 -> ~17 us, conv6_1
            # 23 -> ~10 us: the implicit-GEMM tiles move 2.5 x the bytes per FLOP from L2).  Untimed like the split-K form: a
            # back-to-back burst of these kernels is L2-warm and host-paced.
            ("image", _UNPOOLED, g.k == 1 and image2(g), True, lambda x, w, b: nat.conv2d_image(x, w, b, relu=relu)),
        )
    if igemm_general(g):
        # the extra layers: small maps, one workgroup per CU at most -- the deeper LDS rings (loads three / two steps ahead) hide the L2
        # latency that the two-stage kernel exposes on every K-step
        d, s, p = g.dilation, g.stride, g.padding
        general = lambda v: (lambda x, w, b: nat.conv2d(x, w, b, stride=s, padding=p, dilation=d, relu=relu, variant=v))
        return (
            ("igemm", (INFERENCE, TRAINING), True, False, general(None)),
            ("igemm5", (INFERENCE, TRAINING), True, False, general(5)),
            ("igemm6", (INFERENCE, TRAINING), True, False, general(6)),
            ("splitk", (INFERENCE,), few_tiles(g.batch * out_side(g.h, g) * out_side(g.w, g), g.cout),
             splitk_measured_regime(g) and not on("NO_SPLITK"), general(8)),
            ("halo", (INFERENCE,), halo_strided(g), False,
             lambda x, w, b: nat.conv2d(x, w, b, stride=s, padding=p, dilation=1, relu=relu, variant=7)),
            # round 6: conv6_2 (19 x 19 -> 10 x 10, stride 2) with the image resident in LDS, the strided taps as addresses, one (image,
            # 64 channels) tile of 128 pixels per workgroup: 256 tiles at batch 32 instead of a split-K launch + its reduction
            ("image", (INFERENCE, TRAINING), image2(g), True,
             lambda x, w, b: nat.conv2d_image(x, w, b, stride=s, padding=p, dilation=d, relu=relu)),
        )
    return ()


def candidates(g, relu, context):
    """Ordered {name: (x, w, b) -> y} of the libssdhip forms offered to `context` for a layer of geometry g; empty: none covers it.
    ('miopen' and 'gemm' need the module: the caller adds them.)"""
    return {name: fn for name, contexts, ok, _untimed, fn in _forms(g, relu, context) if ok and context in contexts}


def untimed_choice(g, relu):
    """The form that the inference path takes WITHOUT a timing run, or None.  A back-to-back microbenchmark of the
    image-resident 1 x 1 / strided kernels and of the 5-30 us split-K launches is host-bound and L2-warm and says nothing about them
    inside the step, where they were measured (r03p, graphed step, two A/B pairs: 2.435 -> 2.353 and 2.455 -> 2.378 ms; chain of extra
    layers 178 -> 138 us).  Only at batch >= 16, and only while SSDHIP_CONV / SSDHIP_PREFER leave the choice to the autotune."""
    if not (autotuned() and g.batch >= 16):
        return None
    untimed = {name for name, contexts, ok, untimed, _fn in _forms(g, relu, INFERENCE) if ok and untimed and INFERENCE in contexts}
    return next((name for name in UNTIMED_PRIORITY if name in untimed), None)


def pooled_candidates(g, kernel, stride, pad, ceil_mode):
    """Conv2D(relu) -> MaxPooling2D on the inference path: every plain form followed by the pooling pass, and for a 2 x 2 / stride-2
    pooling the three forms with the pooling in the convolution's epilogue (the full-resolution activation is never written)."""
    pool = lambda fn: (lambda x, w, b: nat.bias_act_maxpool(fn(x, w, b), None, kernel, stride, pad, ceil_mode, relu=False))
    cands = {name: pool(fn) for name, fn in candidates(g, True, POOLED).items()}
    if cands and kernel == 2 and stride == 2 and pad == 0 and (ceil_mode or (g.h % 2 == 0 and g.w % 2 == 0)):
        cands["igemm_pool"] = lambda x, w, b: nat.conv2d_same_pool2(x, w, b, dilation=g.dilation, relu=True)
        if halo(g):
            cands["halo_pool"] = lambda x, w, b: nat.conv3x3_halo(x, w, b, relu=True, pool=True)
        if c64(g):
            cands["c64_pool"] = lambda x, w, b: nat.conv3x3_c64(x, w, b, relu=True, pool=True)
    return cands


def act_key(g, relu):
    """The autotune key of a plain layer (bench.py formats it positionally)."""
    return ("act", (g.batch, g.cin, g.h, g.w), g.cout, g.k, g.dilation, relu, g.stride, g.padding)


# -- the training step's backward and its fused forms (no timing run: the first form that takes the layer) ---------------------------------
def _same3(g):
    return g is not None and g.k == 3 and (g.stride, g.padding, g.dilation) == (1, 1, 1) and g.cin % 64 == 0 and g.cout % 64 == 0


# csrc/ssdhip_wgrad.hip: (name, the geometry's limit, on the device only, switches that turn it off) in the order tried
WGRAD_FORMS = (
    ("grid", _same3, False, ("NO_OWN_WGRAD",)),                                              # the padded position grid: 3 x 3 'same'
    ("pixels", lambda g: g.k == 1 and (g.stride, g.padding) == (1, 0) and g.cin % 128 == 0 and g.cout % 128 == 0, True, ("NO_OWN_WGRAD",)),
    # any other 3 x 3 as a tap-gathered pixel GEMM: fc6's dilation, the strided and the 'valid' extras
    ("taps", lambda g: g.k == 3 and g.cin % 128 == 0 and g.cout % 128 == 0, True, ("NO_OWN_WGRAD", "NO_TAPS_BWD")),
)


def wgrad_forms(g, cuda):
    """The weight-gradient kernels to try, by name: one that declines (None) hands the layer on, at last to the framework."""
    return tuple(name for name, limit, device, off in WGRAD_FORMS if g is not None and limit(g) and (cuda or not device) and not any(map(on, off)))


def dgrad(g, cuda, linked):
    """The layer's data gradient on the forward kernels as (form, launch of the most specific form offered, masked); all None: the framework's.
    form: "same", or "embedded" behind csrc/ssdhip_train.hip's embedding launch (device only; off with the tap-gathered kernels).  masked: the
    slab kernel runs a 'same' layer whose input is linked (`_ReluLink`): its MSK epilogue masks dL/dx by x > 0 ("mask") and sums its channels ("sums")."""
    if not own_dgrad(g) or on("NO_OWN_DGRAD") or not (dgrad_same(g) or (cuda and not on("NO_TAPS_BWD"))):
        return None, None, None
    forms = candidates(dgrad_geometry(g), False, DGRAD)
    name = next(n for n in DGRAD_PRIORITY if n in forms)
    masked = linked and name == "halo" and dgrad_same(g) and not on("NO_MASKED_DGRAD")
    return ("same" if dgrad_same(g) else "embedded"), forms[name], ("mask" if on("NO_MASKED_SUMS") else "sums") if masked else None


def pool_keep(g, cuda):
    """Conv2D(relu) -> MaxPooling2D(2, 2, 'same') of the step as ONE launch that writes the activation AND the pooled map (KEEP): "c64"
    (csrc/ssdhip_conv64.hip: conv1_2 -> pool1), "halo" (csrc/ssdhip_convh.hip: conv2_2 -> pool2, conv3_3 -> pool3) or None."""
    if not (cuda and _same3(g)) or on("NO_POOL_KEEP"):
        return None
    return "c64" if c64(g) else "halo" if halo(g) and not on("NO_HALO_POOL_KEEP") else None


def first_layer_bwd(g, relu, need_x, cuda):
    """csrc/ssdhip_train.hip, conv1_1_bwd_kernel: ReLU mask, bias and weight gradient of the first layer, which has no data gradient, in ONE pass."""
    return bool(relu and not need_x and cuda and first_layer(g) and not on("NO_CONV1_1_BWD"))


def pool_bwd_fused(g):
    """csrc/ssdhip_train.hip, maxpool2_relu_bwd_bias_kernel: 8 channels to a lane, whole pixels to a workgroup of 256 lanes."""
    return g is not None and g.cout % 8 == 0 and 256 % (g.cout // 8) == 0 and not on("NO_FUSED_POOL_BWD")


def conv1_block(g1, g2):
    """csrc/ssdhip_conv64.hip, FRONT: the first layer and the 3 x 3 'same' layer of 64 input channels behind it (conv1_1 -> conv1_2)."""
    return first_layer(g1) and _same3(g2) and c64(g2) and g2.groups == 1 and bool(g2.bias) and not on("NO_CONV1_BLOCK")
