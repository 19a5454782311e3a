"""Case tables and data builders of tests/test_forward_exact_gpu.py: integer (and half-integer) data on which float32 accumulation is
exact in ANY order, so that an inference convolution kernel must return the float64 result of tests/np_conv_forward.py rounded ONCE to
bf16, value for value, and shapes chosen as the smallest that reach each seam of a kernel's work split (the comment of a case names it).

Two kinds of data, both seeded with zlib.crc32(repr(key)):
  * "unit": x, w in {-1, +1}, the bias an integer in -3 .. 3 (or none).  Every partial sum is an integer, every integer up to 256 is a bf16
    number: wherever |want| <= 256 one lost, doubled or misplaced term (+-1 or +-2) changes the output.  At least 99 % of a case's outputs
    (before ReLU) must be there (K <= 4608 gives sigma = sqrt(K) <= 68; `share_within_256` as in tests/backward_exact_cases.py);
  * "rounding": x an integer in -a .. a (a = 8 for K >= 2304, wider for a shorter K -- counting only the taps that can fall inside the
    map -- so that the sums still leave the bf16 integers: `x_amplitude`; 0 .. 255 for the 3-channel images), w in -4 .. 4, the bias a multiple of 0.5 in -3 .. 3 -- per channel the one that puts
    most of the channel's first outputs on a tie that round-to-nearest-even takes upward (`tie_bias`; a single-pixel case has one output
    per channel).  Conditions (tests/test_conv_forward_reference_cpu.py, every case): sum |x||w| + |bias| < 2^22 at every output (acc + bias
    is exact in float32 whatever the order), at least 10 % of the outputs are not bf16 numbers before the rounding, at least 8 are ties that
    nearest-even resolves differently from truncation.  This kind sees a truncating store, a bias added after the rounding, a double
    rounding.
For the chain kernels (conv1_block, conv_chain) rounded integers are integers again: every layer but the last has sparse +-1 filters
(`nnz` non-zeros per filter, the case's choice) and an integer bias, and sum |x||w| < 2^24 holds at every output of every layer.

Where the library exports the plan (ssdhip_conv3x3_halo_plan, ssdhip_conv2d_splitk_workspace_bytes: host arithmetic, no launch) a case
carries the plan numbers that put it on its seam and `check_*_plan` asserts them without a GPU."""
import functools
import zlib

import numpy as np

from tests import np_conv_forward as ref

KINDS = ("unit", "rounding")


# ---- the comparison ---------------------------------------------------------------------------------------------------------------
def same(got, want, what):
    """Equality of values (so -0 equals +0), element for element; the report: how many differ, the first index, got and want there."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    diff = got != want
    n = int(diff.sum())
    if n:
        first = tuple(int(i) for i in np.argwhere(diff)[0])
        msg = "%s: %d of %d elements differ, the first at %s: got %r, want %r" % (what, n, diff.size, first, got[first], want[first])
        print(msg)
        raise AssertionError(msg)
    assert np.array_equal(got, want)


# ---- data -------------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))       # (the same data in every process, unlike hash())


def ints(rng, shape, lo, hi):
    return rng.randint(lo, hi + 1, size=shape).astype(np.float64)


def signs(rng, shape):
    return rng.choice(np.array([-1.0, 1.0]), size=shape)


def share_within_256(want):
    """The share of outputs on which the bf16 comparison sees a change of one unit."""
    return float((np.abs(want) <= 256).mean())


def x_amplitude(k_terms):
    """Rounding data: the range of x for a sum over `k_terms` products, so that sigma = sqrt(K a (a + 1) / 3 * 20 / 3) stays near 600."""
    return int(min(64, 8 * int(np.ceil(np.sqrt(2304.0 / k_terms)))))


def taps_inside(n, stride, pad, dil, k):
    """The largest number of a filter row's k taps that fall inside a map of n pixels at one output (1 for a map under the dilated reach)."""
    outs = range(ref.out_size(n, stride, pad, dil, k))
    return max(sum(0 <= o * stride - pad + t * dil < n for t in range(k)) for o in outs)


def _bits(v):
    v32 = np.asarray(v, dtype=np.float32)
    assert np.array_equal(v32.astype(np.float64), np.asarray(v, dtype=np.float64)), "the exact result must be a float32 number"
    return v32.view(np.uint32)


def bf16_trunc(v):
    """The WRONG rounding a mutation test needs: the upper 16 bits of the float32 kept, the rest dropped."""
    return (_bits(v) & np.uint32(0xffff0000)).view(np.float32).astype(np.float64)


def rounding_stats(v):
    """(share of the values that are not bf16 numbers, number of ties that nearest-even takes away from zero = unlike truncation)."""
    u = _bits(v)
    low = u & np.uint32(0xffff)
    return float((low != 0).mean()), int(((low == 0x8000) & (((u >> np.uint32(16)) & np.uint32(1)) == 1)).sum())


def tie_bias(rng, acc):
    """Per output channel the multiple of 0.5 in -3 .. 3 that puts most of the channel's first 64 outputs on an upward tie (ties between
    candidates broken at random): acc [..., C] -> bias [C]."""
    cand = np.arange(-6, 7) * 0.5
    head = acc.reshape(-1, acc.shape[-1])[:64]
    score = np.zeros((len(cand), acc.shape[-1]))
    for i, c in enumerate(cand):
        u = _bits(head + c)
        score[i] = (((u & np.uint32(0xffff)) == 0x8000) & (((u >> np.uint32(16)) & np.uint32(1)) == 1)).sum(axis=0)
    return cand[np.argmax(score + 0.5 * rng.rand(*score.shape), axis=0)]


def magnitude_bound(x, w, bias, stride, pad, dil):
    """max over the outputs of sum |x||w| + |bias|: below 2^22 every partial sum, and acc + bias, is exact in float32."""
    return float(ref.conv_forward(np.abs(x), np.abs(w), None if bias is None else np.abs(bias), stride, pad, dil).max())


@functools.lru_cache(maxsize=None)
def layer(kind, key, x_shape, cout, k, stride, pad, dil, has_bias):
    """One convolution's operands and exact result: dict(x, w, bias, pre) with pre = conv + bias in float64, before ReLU / pool / rounding.
    Built once per (kind, case): the arrays are shared, nobody writes to them."""
    rng = _rng(kind, *key)
    cin = x_shape[3]
    if kind == "unit":
        x, w = signs(rng, x_shape), signs(rng, (cout, k, k, cin))
        bias = ints(rng, (cout,), -3, 3) if has_bias else None
        pre = ref.conv_forward(x, w, bias, stride, pad, dil)
    else:
        a = x_amplitude(taps_inside(x_shape[1], stride, pad, dil, k) * taps_inside(x_shape[2], stride, pad, dil, k) * cin)
        x = ints(rng, x_shape, 0, 255) if cin == 3 else ints(rng, x_shape, -a, a)
        w = ints(rng, (cout, k, k, cin), -4, 4)
        pre = ref.conv_forward(x, w, None, stride, pad, dil)
        bias = tie_bias(rng, pre) if has_bias else None
        if has_bias:
            pre = pre + bias
    for a_ in (x, w, pre) + ((bias,) if has_bias else ()):
        a_.setflags(write=False)
    return dict(x=x, w=w, bias=bias, pre=pre, geometry=(stride, pad, dil))


def sparse_signs(rng, shape, nnz):
    """[Cout, k, k, Cin] filters with `nnz` entries of +-1 per output channel (all of them if nnz covers the filter), the rest zero."""
    cout, n = shape[0], shape[1] * shape[2] * shape[3]
    if nnz >= n:
        return signs(rng, shape)
    w = np.zeros((cout, n))
    for co in range(cout):
        w[co, rng.choice(n, size=nnz, replace=False)] = signs(rng, (nnz,))
    return w.reshape(shape)


@functools.lru_cache(maxsize=None)
def chained(kind, key, x_shape, spec, nnz):
    """A chain's operands and every layer's exact map: spec = ((k, stride, pad, cout, relu), ...).  Every layer but the last: `nnz` +-1
    entries per filter and a bias in {-1, 0, 1}; the last: dense +-1 (unit) or -4 .. 4 with the tie bias (rounding).
    The LAST layer is kept before its ReLU (the test runs it without and with: `epilogue`), the others as the spec says.
    -> dict(x, layers = [dict(w, bias, stride, pad, dil, relu)], maps = the exact map of every layer, bounds = max sum |x||w| + |bias| of every layer)."""
    rng = _rng(kind, *key)
    cin = x_shape[3]
    if kind == "unit":
        x = signs(rng, x_shape)
    else:
        k, s, p = spec[0][:3]                              # (a one-layer chain is a dense layer: the range of cases.layer)
        a = 255 if len(spec) > 1 else x_amplitude(taps_inside(x_shape[1], s, p, 1, k) * taps_inside(x_shape[2], s, p, 1, k) * cin)
        x = ints(rng, x_shape, 0, 255) if cin == 3 else ints(rng, x_shape, -a, a)
    layers, maps, pres, bounds, cur = [], [], [], [], x
    for i, (k, s, p, cout, relu) in enumerate(spec):
        last = i == len(spec) - 1
        if not last:
            w, bias = sparse_signs(rng, (cout, k, k, cin), nnz), ints(rng, (cout,), -1, 1)    # (a bias of -3 .. 3 per layer would add 4 to every map's energy)
        elif kind == "unit":
            w, bias = signs(rng, (cout, k, k, cin)), ints(rng, (cout,), -3, 3)
        else:
            w = ints(rng, (cout, k, k, cin), -4, 4)
            bias = tie_bias(rng, ref.conv_forward(cur, w, None, s, p, 1))
        l = dict(w=w, bias=bias, stride=s, pad=p, dil=1, relu=bool(relu) and not last)
        pre = ref.conv_forward(cur, w, bias, s, p, 1)
        y = ref.relu(pre) if l["relu"] else pre           # (ref.chain's step: the CPU test asserts ref.chain(x, layers) == maps)
        bounds.append(magnitude_bound(cur, w, bias, s, p, 1))
        layers.append(l)
        pres.append(pre)
        maps.append(y)
        cur, cin = ref.to_bf16(y), cout
    for a_ in [x] + maps + [l["w"] for l in layers] + [l["bias"] for l in layers]:
        a_.setflags(write=False)
    return dict(x=x, layers=layers, maps=maps, pres=pres, bounds=bounds)


def epilogue(pre, relu, pool=False):
    """The exact map a kernel rounds: ReLU, then MaxPooling2D(2, 2, 'same') -- rounding is monotonic, so the rounded maximum is the
    maximum of the rounded values."""
    v = ref.relu(pre) if relu else pre
    return ref.maxpool2_same(v) if pool else v


# ---- plans, from the library's exports --------------------------------------------------------------------------------------------
def _lib():
    from ssd_keras_amd import _native as nat
    return nat.load()


# ---- conv2d_same: variants 1, 4, 5, 6 and None (csrc/ssdhip_conv.hip: tiles of 128 pixels x 64 | 128 channels, K steps of 64 channels) -------
SAME_VARIANTS = (None, 1, 4, 5, 6)
SAME_CASES = [  # B, H, W, Cin, Cout, k, dilation, bias
    (2, 19, 19, 64, 64, 3, 1, True),          # BC = 64; M = 722 = 5 tiles + 82 pixels: a partial last M tile
    (1, 9, 11, 256, 128, 3, 1, True),         # K = 2304 (36 steps), BC = 128, one partial tile
    (2, 10, 7, 64, 256, 3, 1, True),          # W < 32: several image rows in one row group; two channel tiles
    (1, 19, 19, 128, 128, 3, 6, True),        # dilation 6 (fc6): most taps of a border pixel are padding
    (1, 19, 19, 192, 64, 3, 6, True),         # dilation 6, three channel slices, BC = 64
    (3, 5, 5, 256, 128, 1, 1, False),         # 1 x 1, no bias
    (2, 19, 19, 128, 128, 1, 1, True),        # 1 x 1 with two channel slices
    (1, 1, 1, 64, 64, 3, 1, True),            # a single pixel: only the centre tap is inside
    (4, 3, 3, 64, 128, 3, 2, True),           # a map smaller than the dilated reach
]


def same_layer(kind, case):
    b, h, w, cin, cout, k, d, has_bias = case
    return layer(kind, ("same",) + case, (b, h, w, cin), cout, k, 1, d * (k // 2), d, has_bias)


# ---- conv2d: the general entry, variants None, 5, 6 and 8 (split-K) -------------------------------------------------------------------------
GENERAL_VARIANTS = (None, 5, 6, 8)
# Split-K (variant 8): T = k k Cin / 64 steps in `ksplit` = min(ceil(200 / tiles), T, 12) ranges [T r / ksplit, T (r + 1) / ksplit): with
# T = 18 and 12 ranges six of them hold two steps and six one -- the floor bounds put the shorter ranges FIRST, the last is a long one.
# (B, H, W, Cin, Cout, k, stride, pad, dilation, bias) -> (T, ranges, steps of the shortest range, of the longest)
GENERAL_CASES = [
    ((2, 19, 19, 256, 512, 3, 2, 1, 1, True), (36, 12, 3, 3)),   # conv6_2: stride 2 behind padding 1 on an odd map, 19 -> 10; twelve equal ranges
    ((3, 10, 10, 128, 256, 3, 2, 1, 1, True), (18, 12, 1, 2)),   # conv7_2: ... on an even map, 10 -> 5: the last row / column is never tap 0; uneven ranges
    ((3, 5, 5, 128, 256, 3, 1, 0, 1, True), (18, 12, 1, 2)),     # conv8_2: 'valid', 5 -> 3
    ((2, 3, 3, 128, 256, 3, 1, 0, 1, True), (18, 12, 1, 2)),     # conv9_2: 'valid', 3 -> 1: one output pixel per image
    ((2, 32, 32, 128, 256, 3, 2, 1, 1, True), (18, 12, 1, 2)),   # even size 32 -> 16: M = 512 = four full tiles
    ((3, 11, 7, 64, 64, 3, 3, 0, 1, False), (9, 9, 1, 1)),       # stride 3 'valid', rectangular, no bias, BC = 64: one step per range
    ((1, 20, 20, 64, 128, 3, 2, 2, 2, True), (9, 9, 1, 1)),      # dilation 2 with full padding and stride 2
    ((2, 9, 9, 64, 64, 1, 2, 0, 1, True), (1, 1, 1, 1)),         # 1 x 1 stride 2: a single step, split-K has one range
    ((1, 16, 16, 64, 64, 3, 1, 1, 1, True), (9, 9, 1, 1)),       # the 'same' special case through the general entry
    ((1, 13, 13, 64, 64, 3, 1, 0, 2, True), (9, 9, 1, 1)),       # 'valid' with dilation 2: 13 -> 9
]


def general_layer(kind, case):
    b, h, w, cin, cout, k, s, p, d, has_bias = case
    return layer(kind, ("general",) + case, (b, h, w, cin), cout, k, s, p, d, has_bias)


def check_splitk_plan(case, plan):
    b, h, w, cin, cout, k, s, p, d, _ = case
    m = b * ref.out_size(h, s, p, d, k) * ref.out_size(w, s, p, d, k)
    ksplit = _lib().ssdhip_conv2d_splitk_workspace_bytes(b, h, w, cin, cout, k, s, p, d, 0) // (m * cout * 4)
    t = k * k * cin // 64
    sizes = [t * (r + 1) // ksplit - t * r // ksplit for r in range(ksplit)]
    assert (t, ksplit, min(sizes), max(sizes)) == plan, (case, (t, ksplit, min(sizes), max(sizes)))


# ---- conv3x3_cin3: the first layer.  Its tiles are 256 FLATTENED pixels (C1_BP), whatever the row length, read as three strips of the rows
# above, at and below them -- so the seams are a tile that crosses rows and images (a strip then holds the neighbouring image's pixels,
# which the border test must zero), not tile columns.  (Its grid is capped at 1 536 workgroups = 393 216 pixels; no case here, nor
# the 2 x 300 x 300 of tests/test_conv_gpu.py, sends a workgroup to a second tile.) -------------------------------------------------------------
CIN3_CASES = [  # B, H, W
    (3, 7, 5),            # 105 pixels: one partial tile that holds three images of 5-wide rows
    (1, 1, 1),            # one pixel: only the centre tap
    (1, 16, 16),          # one tile exactly
    (2, 33, 64),          # 16.5 tiles of four rows each; the ninth straddles the two images
    (1, 5, 130),          # 2.54 tiles: rows longer than half a tile, tile edges in mid-row
]


def cin3_layer(kind, case):
    b, h, w = case
    return layer(kind, ("cin3",) + case, (b, h, w, 3), 64, 3, 1, 1, 1, True)


# ---- conv2d_same_pool2: the implicit-GEMM kernel with the 2 x 2 pool in its epilogue ----------------------------------------------------------
POOL_CASES = [  # B, H, W, Cin, Cout, k, dilation
    (3, 5, 7, 64, 64, 3, 1),          # odd map: the last window of every row and column is clipped; one partial column tile
    (1, 1, 1, 64, 128, 3, 1),         # a single pixel = a single clipped window
    (2, 8, 130, 64, 64, 1, 1),        # 1 x 1 kernel, three column tiles, the last with two columns
    (1, 19, 19, 128, 64, 3, 2),       # dilation 2
]


def pool_layer(kind, case):
    b, h, w, cin, cout, k, d = case
    return layer(kind, ("pool2",) + case, (b, h, w, cin), cout, k, 1, d * (k // 2), d, True)


# ---- conv2d_same_group, conv3x3_halo_group: problems of different size in one launch ----------------------------------------------------------
# The six predictor-head shapes at batch 2 (B, H, W, Cin, Cout); the slab kernel takes Cout % 128 == 0 only.
GROUP_SHAPES = [(2, 38, 38, 512, 128), (2, 19, 19, 1024, 192), (2, 10, 10, 512, 192), (2, 5, 5, 256, 192), (2, 3, 3, 256, 128), (2, 1, 1, 256, 128)]
SLAB_GROUP_SHAPES = [(2, 38, 38, 512, 128), (2, 19, 19, 1024, 256), (2, 10, 10, 512, 256), (2, 5, 5, 256, 256), (2, 3, 3, 256, 128), (2, 1, 1, 256, 128)]
GROUP_1X1 = (2, 10, 10, 512, 64)          # the 1 x 1 member of the biased launch of conv2d_same_group (on the third head's map size)


def group_layers(kind, shapes, has_bias, one_by_one=None):
    """The members of a grouped launch (K = 9216 of the second head: its sigma = 96 keeps 99 % of ITS outputs within 256 too)."""
    out = [layer(kind, ("group", i, has_bias) + s, s[:4], s[4], 3, 1, 1, 1, has_bias) for i, s in enumerate(shapes)]
    if one_by_one is not None:
        out.append(layer(kind, ("group 1x1",) + one_by_one, one_by_one[:4], one_by_one[4], 1, 1, 0, 1, False))
    return out


# ---- conv3x3_c64 (plain, pool), conv3x3_c64_pool_keep (csrc/ssdhip_conv64.hip: resident filters; one persistent workgroup per CU, 256, walks
# tiles of 16 x 8 or 8 x 16 pixels -- whichever pads less -- per 64-channel output slice) ------------------------------------------------------------
C64_CASES = [  # B, H, W, Cout
    (3, 5, 7, 64),            # a single partial tile per image
    (1, 1, 1, 128),           # a single pixel; two 64-channel output slices
    (2, 9, 130, 64),          # wide and short
    (1, 75, 75, 64),          # odd map: clipped pooling windows, ragged tiles in both directions
    (40, 16, 16, 64),         # two full tiles per image, 80 in all
    (300, 2, 3, 64),          # 300 tiles (one per image) on 256 persistent workgroups: 44 of them walk on to a second tile, whose halo was requested during the first
]


C64_WORKGROUPS = 256          # what _native passes: the device's CU count


def c64_tiles(b, h, w):
    """c64_launch's tile count (no export states it): 16 x 8 or 8 x 16 pixel tiles over W columns and (H + 1) // 2 row pairs, the shape
    with fewer tiles (ties: 16 x 8), per image."""
    ho = (h + 1) // 2
    return b * min(-(-w // 16) * -(-ho // 4), -(-w // 8) * -(-ho // 8))


def c64_layer(kind, case, has_bias=True):
    b, h, w, cout = case
    return layer(kind, ("c64",) + case, (b, h, w, 64), cout, 3, 1, 1, 1, has_bias)


# ---- conv1_block: conv1_1 -> conv1_2 [-> pool1] in one kernel, the 64-channel halo between them recomputed per tile ---------------------------
BLOCK_CASES = [  # B, H, W, Cout of the second layer
    (1, 37, 53, 64),          # odd in both directions
    (3, 16, 16, 64),          # one tile per image
    (2, 7, 150, 64),          # wide: several column tiles, the halo column between them computed twice
    (1, 1, 1, 64),            # one pixel: the halo is all padding -- it must be ZERO, not relu(bias) of the first layer
    (4, 150, 2, 64),          # two columns: every pixel is on a border
    (2, 9, 21, 128),          # a 128-channel second layer (two output slices)
    (300, 2, 3, 64),          # 300 tiles on 256 persistent workgroups: the producer waves compute a second tile's halo while the first is multiplied
]


def block_chain(kind, case):
    """The first layer's filters are dense (27 terms of at most 255: the second layer's sum stays below 2^24 by a margin the CPU test asserts)."""
    b, h, w, cout = case
    return chained(kind, ("block",) + case, (b, h, w, 3), ((3, 1, 1, 64, 1), (3, 1, 1, cout, 1)), 27)


# ---- the slab kernel (csrc/ssdhip_convh.hip): conv3x3_halo, conv2d_same(variant=7), conv3x3_halo_pool_keep, under SSDHIP_CONVH_MODE 128 | 1152 ----
SLAB_MODES = ("128", "1152")
# Geometry 0 = padded position grid in tiles of 256 positions (5 slab pieces up to 30 columns, 6 up to 62, 7 up to 94), 4 = 16 x 16 pixel
# tiles, 5 = 8 x 32; pooled calls always run on 2-D tiles, per image (pitch 0) or -- schedule 1152 -- over the stacked batch with a row
# pitch of H + 1 or H + 2 (even) where that takes fewer tiles.
# (B, H, W, Cin, Cout, bias) -> ((geometry, tiles) un-pooled, (geometry, tiles, pitch) pooled)
SLAB_CASES = [
    ((2, 9, 11, 128, 128, True), ((0, 1), (4, 2, 0))),                # grid, 5 pieces: 240 positions, one partly filled tile
    ((3, 19, 19, 128, 128, True), ((0, 5), (4, 8, 20))),              # grid, 5 pieces: images end inside a tile; pooled: the stack at pitch 20 = H + 1
    ((1, 7, 37, 256, 128, True), ((0, 2), (5, 2, 0))),                # grid, 6 pieces: 304 positions; K = 2304
    ((1, 5, 67, 128, 256, True), ((0, 2), (5, 3, 0))),                # grid, 7 pieces: 408 positions; two channel tiles
    ((1, 25, 100, 128, 128, True), ((4, 14), (4, 14, 0))),            # 16 x 16 tiles (2 x 7): ragged last row and column of tiles
    ((1, 17, 97, 128, 128, True), ((5, 12), (5, 12, 0))),             # 8 x 32 tiles (3 x 4): one row and one column past a tile edge
    ((16, 32, 32, 128, 512, True), ((4, 64), (4, 64, 0))),            # 2-D tiles on a narrow map: one round of 256 units where the grid takes two
    # The kernel's workgroups are persistent, one per CU (256), over tile units = tiles rounded up to 8 x Cout / 128; all of the above fit
    # one round.  72 x 4 = 288 units un-pooled and 112 x 4 = 448 pooled: workgroups take a SECOND tile, requested during the first one's last slice
    ((42, 19, 19, 128, 512, True), ((0, 66), (5, 105, 20))),
]
SLAB_WORKGROUPS = 256
# Pooled only: (B, H, W, Cin, Cout, bias) -> (geometry, tiles, pitch)
SLAB_POOL_CASES = [
    ((6, 20, 20, 128, 128, True), (5, 17, 22)),               # even map: pitch 22 = H + 2, tiles straddle two images
    ((9, 17, 40, 128, 128, True), (4, 33, 18)),               # pitch 18 = rows of a 16 x 16 tile + 2, the smallest gap the stacked form takes
    ((5, 75, 75, 128, 128, True), (4, 120, 76)),              # pitch 76: the last row of tiles leaves the stack
    ((5, 21, 21, 128, 128, False), (4, 14, 22)),              # no bias: with relu=False the float pooling path
    ((5, 2, 2, 128, 128, True), (4, 5, 0)),                   # one window per image
    ((2, 16, 16, 256, 128, True), (4, 2, 0)),                 # exactly one tile per image
]


def slab_layer(kind, case):
    b, h, w, cin, cout, has_bias = case
    return layer(kind, ("slab",) + case, (b, h, w, cin), cout, 3, 1, 1, 1, has_bias)


def check_slab_plan(case, pooled, plan):
    from ssd_keras_amd import _native as nat
    b, h, w, cin, cout, _ = case
    got = nat.conv3x3_halo_plan(b, h, w, pooled, cout)
    got = got[:3] if pooled else got[:2]
    assert got == plan, (case, pooled, got)


# conv2d(..., variant=7): the slab kernel's stride-1 'same' result on the position grid, the strided / cropped positions kept
SLAB_STRIDED_CASES = [  # B, H, W, Cin, Cout, stride, pad
    (3, 11, 7, 128, 128, 1, 1),           # 'same' through the strided entry
    (1, 20, 20, 256, 128, 2, 0),          # stride 2 'valid' on an even map: 20 -> 9
    (2, 9, 94, 128, 128, 1, 0),           # 'valid' on the widest map: the first and last row and column are cropped
    (2, 19, 19, 256, 128, 2, 1),          # conv6_2: stride 2 behind padding 1
    (456, 5, 5, 128, 512, 1, 0),          # conv8_2 at a batch whose 456 x 36 positions make 65 tiles: 72 x 4 = 288 units, a second round of the 256 persistent workgroups
]


def slab_strided_layer(kind, case):
    b, h, w, cin, cout, s, p = case
    return layer(kind, ("slab strided",) + case, (b, h, w, cin), cout, 3, s, p, 1, True)


# ---- the image-resident kernel (csrc/ssdhip_convimg.hip): conv3x3_image ('same', any dilation), conv2d_image (general) ---------------------------
IMAGE_CASES = [  # B, H, W, Cin, Cout, k, stride, pad, dilation
    (2, 19, 19, 512, 128, 3, 1, 6, 6),        # fc6: dilated taps as addresses, K = 4608
    (3, 10, 10, 256, 128, 3, 1, 1, 1),        # a 100-pixel map: the one-block tile
    (3, 19, 19, 1024, 128, 1, 1, 0, 1),       # 1 x 1 on 361 pixels, 16 slices: three 128-pixel tiles by default (the last holds 105), whole-image
                                              # tiles under SSDHIP_CONVIMG_PXT=0 -- both are run
    (3, 19, 19, 256, 128, 3, 2, 1, 1),        # conv6_2: strided 128-pixel tile, 19 -> 10
    (3, 10, 10, 128, 256, 3, 2, 1, 1),        # conv7_2: 10 -> 5, two channel tiles
]


def image_layer(kind, case):
    b, h, w, cin, cout, k, s, p, d = case
    return layer(kind, ("image",) + case, (b, h, w, cin), cout, k, s, p, d, True)


# ---- conv_chain (csrc/ssdhip_chain.hip): the extra-layer tail in one launch, the maps between the layers in LDS -----------------------------------
# (B, H, W, C0, ((k, stride, pad, cout, relu, keep), ...), non-zeros per filter of every layer but the last for (unit, rounding) data).
# Six layers deep, a ReLU halves a map's energy and n non-zeros multiply it by n: two keep the last map of unit data within +-256,
# three let the maps of rounding data grow past the bf16 integers while the last sum stays far below 2^22.
CHAIN_CASES = [
    (3, 10, 10, 512, ((1, 1, 0, 128, 1, 0), (3, 2, 1, 256, 1, 1), (1, 1, 0, 128, 1, 0), (3, 1, 0, 256, 1, 1), (1, 1, 0, 128, 1, 0),
                      (3, 1, 0, 256, 1, 1)), (2, 3)),                              # the SSD300 tail conv7_1 ... conv9_2: stride 2, 'valid', kept and discarded maps
    (2, 7, 5, 128, ((3, 1, 1, 128, 0, 1), (1, 1, 0, 96, 1, 1)), (8, 8)),            # 'same' padding, no ReLU, 96 output channels, every map kept
    (1, 4, 4, 256, ((3, 2, 1, 32, 1, 1),), (0, 0)),                                 # one layer, 32 output channels
]


def chain_chain(kind, case):
    b, h, w, c0, spec, nnz = case
    return chained(kind, ("chain",) + case, (b, h, w, c0), tuple(l[:5] for l in spec), nnz[KINDS.index(kind)])
