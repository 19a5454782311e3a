"""Case tables and data builders of tests/test_backward_exact_gpu.py: integer data on which float32 accumulation is exact in ANY order,
so that a backward kernel of the training step must return the float64 result of tests/np_conv_grads.py bit for bit (rounded once
where the output is bf16), and shapes chosen as the smallest that reach each seam of a kernel's work split.

Every case carries the plan numbers that make it reach its seam; `check_*_plan` recomputes them from what the library exports
(`ssdhip_*_workspace_bytes` / the size of one partial tile = the number of partial slots, `ssdhip_conv3x3_halo_plan`,
`ssdhip_relu_bwd_bias_blocks`, `ssdhip_conv1_1_bwd_blocks` -- host arithmetic, no launch) and asserts them, so a change of a plan
that moves a case off its seam fails tests/test_conv_grads_reference_cpu.py without a GPU.

Data conditions (asserted by the same CPU test for every case):
  * weight gradients (float32 out): x in {+-1, +-2, +-3}, dy in {+-1, +-2}, no zeros.  |term| <= 6, so with positions x 6 < 2^24 every
    partial and every final sum is an integer below 2^24: exact in float32 whatever the order;
  * data gradients (bf16 out): dy, w in {-1, +1}.  The sum over K terms is an integer of K's parity; every integer up to 256 is a bf16
    number, so wherever |want| <= 256 one lost or doubled term (+-1 or +-2) shows.  At least 99 % of a case's outputs must be there
    (K <= 4608); beyond, the result is still the exact sum rounded once, only less sensitive;
  * activations for the masks: {0, 1, 2} with about 40 % zeros (no -0, no NaN: tests/test_train_glue_gpu.py owns those)."""
import zlib

import numpy as np

from tests import np_conv_grads as ref


# ---- data -----------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))       # (the same data in every process, unlike hash())


def ints(rng, shape, values):
    return rng.choice(np.asarray(values, dtype=np.float64), size=shape)


def wgrad_data(case, x_shape, dy_shape):
    """(x, dy) of a weight-gradient case: NHWC float64 arrays of small non-zero integers."""
    rng = _rng("wgrad", *case)
    return ints(rng, x_shape, [-3, -2, -1, 1, 2, 3]), ints(rng, dy_shape, [-2, -1, 1, 2])


def wgrad_exact(n_positions, max_term=6):
    """The float32 condition of a sum over `n_positions` products of magnitude <= max_term."""
    return n_positions * max_term < 2 ** 24


def dgrad_data(case, dy_shape, w_shape):
    """(dy, w) of a data-gradient case: entries -1 / +1."""
    rng = _rng("dgrad", *case)
    return ints(rng, dy_shape, [-1, 1]), ints(rng, w_shape, [-1, 1])


def activation(case, shape):
    """A ReLU output for the masks: 0 (40 %), 1, 2."""
    return _rng("act", *case).choice(np.array([0.0, 1.0, 2.0]), size=shape, p=[0.4, 0.3, 0.3])


def share_within_256(want):
    """The share of outputs on which the bf16 comparison sees a change of one unit."""
    return float((np.abs(want) <= 256).mean())


def flipped(w):
    """[Cout, k, k, Cin] filters -> the data gradient's [Cin, k, k, Cout]: transposed, taps flipped."""
    return np.ascontiguousarray(w[:, ::-1, ::-1, :].transpose(3, 1, 2, 0))


# ---- plans, from the library's exports ------------------------------------------------------------------------------------------
def _lib():
    from ssd_keras_amd import _native as nat
    return nat.load()


def _ceil(a, b):
    return -(-a // b)


def pixel_split_plan(n_pixels, splits):
    """(steps of 64 pixels, splits, steps of the last split, pixels of the last step) of the two pixel-GEMM weight gradients."""
    n_steps = _ceil(n_pixels, 64)
    per = _ceil(n_steps, splits)
    assert _ceil(n_steps, per) == splits
    return n_steps, splits, n_steps - (splits - 1) * per, n_pixels - (n_steps - 1) * 64


# 1 x 1 weight gradient (wg1_plan: splits = min(512 / tiles, steps), lowered until a split has >= 4 steps, so more than one split
# needs >= 8 steps = 449 pixels).  (B, H, W, Cin, Cout) -> (steps, splits, steps of the last split, pixels of the last step)
WG1_CASES = [
    ((1, 11, 47, 128, 128), (9, 2, 4, 5)),        # 517 pixels: splits of 5 and 4 steps, the last step holds 5 pixels
    ((2, 16, 16, 128, 128), (8, 2, 4, 64)),       # 512 pixels: an exact multiple of 64, two full splits
    ((1, 11, 47, 256, 256), (9, 2, 4, 5)),        # two ci tiles x two co tiles over the same seam
    ((2, 3, 137, 128, 256), (13, 4, 1, 54)),      # 822 pixels: four splits of 4, 4, 4 and 1 steps, the last of 54 pixels
    ((1, 1, 1, 128, 128), (1, 1, 1, 1)),          # one pixel: 63 of the step's 64 rows are padding
]


def check_wg1_plan(case, plan):
    b, h, w, cin, cout = case
    splits = _lib().ssdhip_conv1x1_wgrad_workspace_bytes(b * h * w, cin, cout) // (cout * cin * 4)
    assert pixel_split_plan(b * h * w, splits) == plan, (case, pixel_split_plan(b * h * w, splits))


# Tap-gathered weight gradient (wgt_plan: the same split rule over the OUTPUT pixels, tiles = 3 filter rows per (co, ci) tile).
# (B, H, W, Cin, Cout, stride, pad, dilation) -> the pixel plan.  The input maps are as small as 517 (or about as many) output pixels allow.
TAP_CASES = [
    ((1, 21, 93, 128, 128, 2, 1, 1), (9, 2, 4, 5)),      # stride 2 behind padding 1, odd map -> 11 x 47: the last tap row / column is inside
    ((1, 22, 94, 128, 128, 2, 1, 1), (9, 2, 4, 5)),      # ... even map -> 11 x 47: the last input row / column is never read by tap 0
    ((1, 13, 49, 128, 128, 1, 0, 1), (9, 2, 4, 5)),      # 'valid' -> 11 x 47
    ((1, 34, 142, 128, 128, 3, 0, 1), (9, 2, 4, 5)),     # stride 3 'valid' -> 11 x 47, one unused input row and column
    ((1, 11, 47, 128, 256, 1, 2, 2), (9, 2, 4, 5)),      # dilation 2 behind padding 2 -> 11 x 47, two co tiles
    ((58, 3, 3, 128, 128, 1, 2, 2), (9, 2, 4, 10)),      # 3 x 3 map under a reach of 5: every tap but the centre is partly outside; 522 pixels
    ((2, 6, 7, 256, 128, 2, 0, 1), (1, 1, 1, 12)),       # stride 2 'valid' -> 2 x 3: one step, two ci tiles
    ((1, 10, 66, 128, 128, 1, 0, 1), (8, 2, 4, 64)),     # 'valid' -> 8 x 64 = 512 pixels: an exact multiple of 64, two full splits
    ((1, 13, 49, 256, 256, 1, 0, 1), (9, 2, 4, 5)),      # two ci tiles x two co tiles (x three filter rows) over the 517-pixel seam
    ((1, 3, 3, 128, 128, 1, 0, 1), (1, 1, 1, 1)),        # one output pixel
]


def tap_out_shape(case):
    b, h, w, cin, cout, s, p, d = case
    return b, ref.out_size(h, s, p, d, 3), ref.out_size(w, s, p, d, 3), cout


def check_tap_plan(case, plan):
    b, h, w, cin, cout, s, p, d = case
    _, ho, wo, _ = tap_out_shape(case)
    splits = _lib().ssdhip_conv3x3_taps_wgrad_workspace_bytes(b, h, w, cin, ho, wo, cout, s, p, d) // (cout * 9 * cin * 4)
    assert pixel_split_plan(b * ho * wo, splits) == plan, (case, pixel_split_plan(b * ho * wo, splits))


# Position-grid weight gradient (wg_plan): image b, row h, column w is position (b (H + d) + h)(W + d) + w of a padded grid, streamed in
# blocks of 64 positions; `splits` (a multiple of 8, 8 until a split would still get 12 blocks) workgroups per tile take
# ceil(blocks / splits) blocks each, a split past the end writes a zero tile.  Cout % 128 == 0: one partial slot per split; Cout = 64:
# two (the two K halves of every block).  (B, H, W, Cin, Cout) -> (blocks, splits, slots, splits with work, blocks of the last of them)
GRID_CASES = [
    ((1, 5, 7, 64, 128), (1, 8, 8, 1, 1)),          # 48 positions in one block: seven idle splits; W < 8, eight row wraps in the block
    ((2, 13, 6, 64, 128), (4, 8, 8, 4, 1)),         # W < 8 on a map taller than a block: nine row wraps per block, four idle splits
    ((1, 1, 1, 64, 128), (1, 8, 8, 1, 1)),          # one pixel: eight of the nine taps see only padding
    ((2, 19, 19, 128, 128), (13, 8, 8, 7, 1)),      # 13 blocks in splits of 2: the seventh split is short, the eighth idle; two ci tiles
    ((3, 7, 9, 64, 64), (4, 8, 16, 4, 1)),          # Cout = 64: two K halves per block, sixteen slots
    ((2, 19, 19, 128, 64), (13, 8, 16, 7, 1)),      # ... with a short last split and two ci tiles
    ((1, 3, 190, 64, 128), (12, 8, 8, 6, 2)),       # the widest map of the 128-channel form: three halo blocks, the ring wraps
    ((1, 2, 318, 64, 64), (15, 8, 16, 8, 1)),       # the widest map of the 64-channel form: five halo blocks, a short last split
    ((8, 38, 38, 128, 128), (191, 16, 16, 16, 11)),  # the smallest batch of a 38 x 38 map with sixteen splits (12 blocks each, the last 11)
]

# ... and its dilated form (fc6: dilation 6, Cout % 128 == 0) through conv3x3_taps_wgrad, which also runs the same geometry on the
# tap-gathered kernel under SSDHIP_WGRAD_GATHER_ONLY=1.  (B, H, W, Cin, Cout) -> the grid plan with d = 6
DILATED_CASES = [
    ((1, 19, 19, 128, 128), (10, 8, 8, 5, 2)),      # 25 x 25 positions per image: five splits of two blocks, three idle
    ((2, 19, 19, 128, 256), (20, 8, 8, 7, 2)),      # two images, two co tiles: splits of three blocks, the seventh has two
    ((26, 5, 4, 128, 128), (45, 8, 8, 8, 3)),       # a map smaller than the reach of 12: only the centre tap is ever inside; 520 pixels
]


def grid_plan(case, slots, dil=1):
    b, h, w, cin, cout = case
    splits = slots // (1 if cout % 128 == 0 else 2)
    blocks = _ceil(b * (h + dil) * (w + dil), 64)
    per = _ceil(blocks, splits)
    used = _ceil(blocks, per)
    return blocks, splits, slots, used, blocks - (used - 1) * per


def check_grid_plan(case, plan):
    b, h, w, cin, cout = case
    slots = _lib().ssdhip_conv3x3_wgrad_workspace_bytes(b, h, w, cin, cout) // (cout * 9 * cin * 4)
    assert grid_plan(case, slots) == plan, (case, grid_plan(case, slots))


def check_dilated_plan(case, plan):
    """The taps entry reserves the larger of the two kernels' scratch: eight slots mean the position grid (the gather kernel splits a
    few hundred pixels in two)."""
    b, h, w, cin, cout = case
    slots = _lib().ssdhip_conv3x3_taps_wgrad_workspace_bytes(b, h, w, cin, h, w, cout, 1, 6, 6) // (cout * 9 * cin * 4)
    assert grid_plan(case, slots, 6) == plan, (case, grid_plan(case, slots, 6))


# ReLU mask + channel sums (relu_bwd_bias_kernel): a workgroup has 256 / (C / 8) pixel lanes, workgroup g takes pixels
# g lanes + lane, + blocks lanes, ...  517 pixels leave the last sweep's last workgroup with some lanes empty at every C.
# (pixels as (B, H, W), C) -> (workgroups, pixel lanes, pixels of the last sweep)
MASK_CASES = [
    ((1, 11, 47, 64), (3, 32, 37)),
    ((1, 11, 47, 128), (5, 16, 37)),
    ((1, 11, 47, 512), (17, 4, 41)),
    ((1, 11, 47, 1024), (33, 2, 55)),
]


def check_mask_plan(case, plan):
    b, h, w, c = case
    n = b * h * w
    blocks = _lib().ssdhip_relu_bwd_bias_blocks(n, c)
    lanes = 256 // (c // 8)
    got = (blocks, lanes, n % (blocks * lanes))
    assert got == plan and got[2] % lanes != 0 and blocks > 1, (case, got)


# Data gradient of a 3 x 3 'same' layer through the slab kernel (conv3x3_halo_plan: geometry 0 = padded position grid in tiles of
# 256 positions, run with 5 slab pieces up to 30 columns, 6 up to 62, 7 up to 94; 4 = 16 x 16 pixel tiles, 5 = 8 x 32, taken beyond
# 94 columns -- whichever needs fewer tiles, ties to 16 x 16 -- or where they finish in fewer rounds of 256 workgroups).
# (B, H, W, gradient channels, input channels) -> (geometry, tiles)
SLAB_CASES = [
    ((2, 9, 11, 128, 128), (0, 1)),                 # grid, 5 pieces: 240 positions, one partly filled tile
    ((3, 19, 19, 128, 128), (0, 5)),                # grid, 5 pieces: several tiles, images end inside a tile
    ((1, 7, 37, 256, 128), (0, 2)),                 # grid, 6 pieces: 304 positions; K = 2304
    ((1, 5, 67, 128, 256), (0, 2)),                 # grid, 7 pieces: 408 positions; two channel tiles
    ((1, 25, 100, 128, 128), (4, 14)),              # 16 x 16 tiles (2 x 7 against 4 x 4 of 8 x 32): ragged last row and column of tiles
    ((1, 17, 97, 128, 128), (5, 12)),               # 8 x 32 tiles (3 x 4 against 2 x 7): one row and one column past a tile edge
    ((16, 32, 32, 128, 512), (4, 64)),              # 2-D tiles on a narrow map: 64 x 4 = 256 units in one round, the grid's 69 x 4 take two
]


def check_slab_plan(case, plan):
    from ssd_keras_amd import _native as nat
    b, h, w, cy, cx = case
    got = nat.conv3x3_halo_plan(b, h, w, False, cx)[:2]
    assert got == plan, (case, got)


# Data gradient through the other forward kernels.  (B, H, W, gradient channels, input channels, k, dilation, kernels)
FORWARD_CASES = [
    (2, 9, 70, 64, 64, 3, 1, ("same", "c64")),            # a 64-channel gradient (conv1_2): K = 576; 70 columns cross a 64-column tile
    (2, 19, 19, 512, 128, 3, 6, ("same", "image")),       # fc6's data gradient: dilation 6 at 19 x 19, K = 4608
    (3, 10, 10, 256, 128, 3, 1, ("same", "image")),       # a small map on the image-resident kernel
    (2, 19, 19, 1024, 128, 1, 1, ("same",)),              # a 1 x 1 layer: K = 1024
]

# Strided and 'valid' 3 x 3 layers through models._common._conv_input_weight_grads: (B, H, W, Cin, Cout, stride, pad)
STRIDED_CASES = [
    (3, 7, 9, 128, 128, 2, 1),
    (2, 10, 10, 128, 256, 2, 1),
    (3, 5, 5, 128, 128, 1, 0),
    (4, 3, 3, 256, 128, 1, 0),
    (2, 8, 6, 128, 128, 3, 0),
]

# conv1_1's one-pass backward: a workgroup takes tiles of 64 columns of one image row.  (B, H, W) -> workgroups = min(B H ceil(W / 64), 1024)
FIRST_LAYER_CASES = [
    ((1, 1, 1), 1),
    ((2, 5, 130), 30),            # three tiles per row, the last two columns wide
    ((3, 37, 41), 111),
    ((1, 3, 64), 3),              # exactly one tile per row
    ((3, 350, 5), 1024),          # 1 050 tiles on the launch's cap of 1 024 workgroups: 26 of them take a second tile
]


def check_first_layer_plan(case, blocks):
    assert _lib().ssdhip_conv1_1_bwd_blocks(*case) == blocks, case


# One 128 -> 128 layer as the training step runs it: the masked data gradient of the layer above with its channel sums, then this
# layer's weight gradient with those sums as its bias partials.  (B, H, W, C)
CHAIN_CASE = (2, 19, 19, 128)
