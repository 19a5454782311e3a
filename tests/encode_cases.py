"""Ground truth for the encoder kernels (csrc/ssdhip_encode.hip) built straight from NumPy: tests/test_encode_cases_cpu.py checks
every claim made here against the oracle alone, tests/test_encode_paths_gpu.py runs the table on the device, and
tests/golden/make_golden.py pins the oracle on it with the reference (tests/golden/encoder_edges.npz).

The DYADIC configuration makes ties real.  A 128 x 128 image, three predictor layers of square anchors, absolute coordinates and
unit variances: every anchor corner is a multiple of 4 and every IoU of a box on the 4-pixel grid is a ratio of small integers, many
of them exact binary fractions -- equal IoUs are equal bit for bit, and 0.5 and 0.25 are hit exactly.  N = 336 anchors, n = index:

    layer 0   16 x 16 anchors of 16 x 16 px   n = 16 i + j            x in [8 j - 4, 8 j + 12], y likewise with i     n =   0 .. 255
    layer 1    8 x  8 anchors of 32 x 32 px   n = 256 + 8 i + j       x in [16 j - 8, 16 j + 24]                      n = 256 .. 319
    layer 2    4 x  4 anchors of 64 x 64 px   n = 320 + 4 i + j       x in [32 j - 16, 32 j + 48]                     n = 320 .. 335

rowmax_kernel and finalize_kernel<TA = 256> see layer 0 as tile 0 (four waves of 64 lanes, n // 64) and the rest as a partial tile 1
(n // 256); match_kernel's re-scan deals anchor n to thread n of its 1024, so there too n // 64 is the wave.

A Case is (config overrides, ground truth list, claims).  A claim says which tie or threshold hit the case is FOR; the CPU test
recomputes it from `orc.iou`.  `breaks` lists the (coords, border_pixels) combinations under which a claim does not hold (the case
still runs there on the device: it is then an ordinary case) -- a case cannot silently lose its tie.  Everything returned is computed
once per process and must be left unchanged by whoever uses it."""
import functools

import numpy as np

from oracle import np_oracle as orc

DYADIC = dict(img_height=128, img_width=128, n_classes=5, predictor_sizes=[(16, 16), (8, 8), (4, 4)], scales=[0.125, 0.25, 0.5, 1.0],
              aspect_ratios_global=[1.0], two_boxes_for_ar1=False, steps=None, offsets=None, clip_boxes=False,
              variances=[1.0, 1.0, 1.0, 1.0], normalize_coords=False, coords="corners", border_pixels="half", matching_type="multi",
              pos_iou_threshold=0.5, neg_iou_limit=0.25)
N_ANCHORS = 336
# the same layers with a 3 x 3 map on top: N = 329 is odd, so with an odd row length the images of a batch (and the tiles of an image)
# start on different 16-byte phases of a float32 output.  N = 336 cannot show that: 336 and every tile start are multiples of 4.
ODD_N = dict(DYADIC, predictor_sizes=[(16, 16), (8, 8), (3, 3)])
N_ANCHORS_ODD = 329

COORDS = ("corners", "centroids", "minmax")
BORDERS = ("half", "include", "exclude")
MATCHING = ("multi", "bipartite")
SIZE_BREAKS = frozenset((c, b) for c in COORDS for b in ("include", "exclude"))     # a tie between anchors of DIFFERENT size needs d = 0
EXCLUDE_BREAKS = frozenset((c, "exclude") for c in COORDS)      # d = -1 shrinks the areas: the IoUs end up ABOVE the thresholds

# sizeof(GtBox) in csrc/ssdhip_encode.hip: double lab[4] (32) + PxBox<double> {x0, y0, x1, y1, area} (40) + int cls (4), padded to the
# 8-byte alignment of its doubles.  The launcher's dynamic LDS for match_kernel is
#     m_lds = max_gt * (sizeof(GtBox) + sizeof(double) + 3 * sizeof(int)) + ceil(N / 32) * 4 + 16
# and above 48 KiB it has to raise the kernel's limit with hipFuncSetAttribute first.
GTBOX_BYTES = 80
ENC_MAX_GT = 1024


def match_lds_bytes(max_gt, n_anchors=N_ANCHORS):
    return max_gt * (GTBOX_BYTES + 8 + 12) + (n_anchors + 31) // 32 * 4 + 16


G48 = next(g for g in range(1, ENC_MAX_GT + 1) if match_lds_bytes(g) > 48 * 1024)      # the smallest box count past 48 KiB
LADDER = (1, 63, 64, 65, 256, 257, G48 - 1, G48, ENC_MAX_GT)


def finalize_tile(L, esz):
    """The launcher's tile rule: TA halves from 256 to 64 while TA * L * esz exceeds 36 KiB."""
    ta = 256
    while ta > 64 and ta * L * esz > 36 * 1024:
        ta >>= 1
    return ta


# C incl. background -> (L, float32 TA, float64 TA); C = 5 is the odd row length
CLASS_TABLE = {6: (18, 256, 256), 21: (33, 256, 128), 41: (53, 128, 64), 81: (93, 64, 64), 5: (17, 256, 256)}


def _gt(*rows):
    return np.array(rows, dtype=np.float64).reshape(-1, 5)


EMPTY = np.zeros((0, 5))
FAR = [200.0, 200.0, 210.0, 212.0]              # outside every anchor: an all-zero row of the similarity matrix

# boxes named after the anchors they tie on
LANES = [8.0, 44.0, 24.0, 60.0]                 # 0.6 at 97, 98: row 6, columns 1 and 2 -- two lanes of wave 1
LANES_R = [16.0, 44.0, 32.0, 60.0]              # 0.6 at 98, 99
WAVES = [36.0, 24.0, 52.0, 40.0]                # 0.6 at 53, 69: midway between anchor rows 3 (wave 0) and 4 (wave 1), column 5
TILES = [8.0, 12.0, 40.0, 28.0]                 # 0.5 at 34, 35 (tile 0) and 265 (tile 1)
FOUR = [40.0, 24.0, 56.0, 40.0]                 # 9/23 at 53, 54 (wave 0), 69, 70 (wave 1): midway in x and in y
FULL = [0.0, 0.0, 128.0, 128.0]                 # 0.25 at 325, 326, 329, 330, the four 64 x 64 anchors inside the image
ABOVE = [12.0, 40.0, 28.0, 56.0]                # 0.6 at 82, 98: midway between rows 5 and 6, column 2
CORNER = [0.0, 0.0, 12.0, 12.0]                 # 0.5625 at anchor 0 alone


class Case:
    """claims: ("row", image, row, columns, distance) -- the row's maximum is attained at exactly `columns`; distance "lane": the
                   first two share n // 64, "wave": n // 64 differs inside one n // 256, "tile": n // 256 differs
               ("rows", image, (r, s), same_column) -- rows r < s have equal maxima, their first columns equal or not
               ("rescan", image, row, taken, columns, distance) -- with the columns `taken` zeroed the row's maximum is at `columns`
               ("column", image, anchor, (r, s)) -- the anchor's maximum over rows is attained at exactly r and s, it is no row's
                   first column (no bipartite match), and the value reaches pos_iou_threshold
               ("claimed", image, anchor, rows) -- the bipartite matching assigns `anchor` to every row of `rows`
               ("zero_row", image, row) -- the row overlaps no anchor
               ("on_pos", image, row, columns) / ("on_neg", ...) -- the IoU equals the threshold bit for bit
               ("only_bipartite", image) -- with these thresholds no anchor but the g bipartite ones is matched, none is neutral"""

    def __init__(self, name, gt, purpose, claims=(), breaks=frozenset(), base=None, **over):
        self.name, self.purpose, self.claims, self.breaks, self.over = name, purpose, tuple(claims), frozenset(breaks), over
        self.base = DYADIC if base is None else base
        self.gt = [np.array(g, dtype=np.float64).reshape(-1, 5) for g in gt]
        for g in self.gt:
            g.setflags(write=False)

    def __repr__(self):
        return self.name

    def config(self, **over):
        return dict(dict(self.base, **self.over), **over)

    def holds(self, coords, border):
        return (coords, border) not in self.breaks

    def oracle(self, **over):
        """(y float64 (B, N, C + 12), match map int32 (B, N)) of the oracle under config(**over); read-only, computed once."""
        return _oracle(self, tuple(sorted(over.items())))


@functools.lru_cache(maxsize=None)
def _oracle(case, over):
    with np.errstate(invalid="ignore", divide="ignore"):
        y, mm = orc.EncoderOracle(**case.config(**dict(over)))(case.gt, return_matches=True)
    y.setflags(write=False)
    mm.setflags(write=False)
    return y, mm


def similarities(case, image, **over):
    """The (g, N) IoU matrix the encoder builds for one image (ssd_input_encoder.py:339-352), from the oracle's pieces."""
    kw = case.config(**over)
    ora = orc.EncoderOracle(**kw)
    lab = np.array(case.gt[image], dtype=np.float64)
    if kw["normalize_coords"]:
        lab[:, [2, 4]] /= kw["img_height"]
        lab[:, [1, 3]] /= kw["img_width"]
    if kw["coords"] == "centroids":
        lab = orc.convert_coordinates(lab, 1, "corners2centroids", kw["border_pixels"])
    elif kw["coords"] == "minmax":
        lab = orc.convert_coordinates(lab, 1, "corners2minmax")
    return orc.iou(lab[:, 1:5], ora.anchors(), coords=kw["coords"], mode="outer_product", border_pixels=kw["border_pixels"])


def _integer_boxes(g, n_classes, seed):
    """g boxes of 4..28 px with integer corners inside the image: IoUs are ratios of small integers, so ties between DIFFERENT boxes
    happen too, and the encoded offsets are short binary fractions (the golden file stays small)."""
    rng = np.random.RandomState(seed)
    w, h = rng.randint(4, 29, size=g), rng.randint(4, 29, size=g)
    x0, y0 = rng.randint(0, 128 - 28, size=g), rng.randint(0, 128 - 28, size=g)
    return np.stack([rng.randint(1, n_classes + 1, size=g), x0, y0, x0 + w, y0 + h], axis=1).astype(np.float64)


def random_boxes(g, n_classes, seed, identical=8):
    """g float boxes of 4..28 px; from 16 boxes on, the last `identical` (at most 8: many identical boxes make the bipartite re-scan
    quadratic) are copies of the first."""
    assert identical <= 8
    rng = np.random.RandomState(seed)
    w, h = rng.uniform(4, 28, size=g), rng.uniform(4, 28, size=g)
    x0, y0 = rng.uniform(0, 100, size=g), rng.uniform(0, 100, size=g)
    gt = np.stack([rng.randint(1, n_classes + 1, size=g).astype(np.float64), x0, y0, x0 + w, y0 + h], axis=1)
    if g >= 16:
        gt[g - (identical - 1):, 1:] = gt[0, 1:]
    return gt


TIES = [
    Case("row_tie_lanes", [_gt([1] + LANES)], "row maximum tied between two lanes of one wave: the first column wins in wave_argmax",
         [("row", 0, 0, (97, 98), "lane")]),
    Case("row_tie_waves", [_gt([2] + WAVES)], "row maximum tied between waves 0 and 1 of tile 0: match_kernel's reduce of the partials",
         [("row", 0, 0, (53, 69), "wave")]),
    Case("row_tie_tiles", [_gt([3] + TILES)], "row maximum tied between tile 0 and the partial tile 1",
         [("row", 0, 0, (34, 35, 265), "tile")], breaks=SIZE_BREAKS),
    Case("rows_tie_other_columns", [_gt([1] + LANES_R, [2] + WAVES, [3] + LANES)],
         "three rows with equal maxima 0.6 in different columns: the rounds take them lowest row first",
         [("rows", 0, (0, 1), False), ("rows", 0, (1, 2), False)]),
    Case("duplicate_boxes", [_gt([1] + LANES, [2] + LANES, [3] + LANES)],
         "identical rows: equal maxima in ONE column; the later rows are re-scanned with the taken columns masked",
         [("rows", 0, (0, 1), True), ("rows", 0, (1, 2), True), ("rescan", 0, 1, (97,), (98,), "lane")]),
    Case("rescan_tie_waves", [_gt([1] + FOUR, [2] + FOUR)],
         "the re-scanned row's new maximum is tied between wave 0 (54) and wave 1 (69, 70)",
         [("row", 0, 0, (53, 54, 69, 70), "wave"), ("rows", 0, (0, 1), True), ("rescan", 0, 1, (53,), (54, 69, 70), "wave")]),
    Case("multi_tie_two_boxes", [_gt([4] + ABOVE, [5] + LANES)],
         "anchor 98 has IoU 0.6 with both boxes and is neither's bipartite match: the multi match keeps the FIRST box",
         [("column", 0, 98, (0, 1))], pos_iou_threshold=0.375),        # (0.497 under 'include': a threshold all borders reach)
]

QUIRKS = [
    Case("column_claimed_twice", [_gt([1] + CORNER, [2] + FAR)],
         "row 1 overlaps nothing and keeps anchor 0, which row 0 matched: the highest row's class and box are written",
         [("claimed", 0, 0, (0, 1)), ("zero_row", 0, 1)]),
    Case("zero_row_first", [_gt([3] + FAR, [1] + WAVES, [2] + CORNER)], "a box that overlaps no anchor as row 0",
         [("zero_row", 0, 0), ("claimed", 0, 0, (0, 2))]),
    Case("zero_row_last", [_gt([1] + WAVES, [2] + LANES, [3] + FAR)],
         "a box that overlaps no anchor as the last row: the all-zero last round gives anchor 0 to row 0, which loses anchor 53",
         [("zero_row", 0, 2), ("claimed", 0, 0, (0, 2))]),
    Case("more_boxes_than_anchors", [EMPTY, _integer_boxes(N_ANCHORS + 4, 5, 11), _gt([1] + TILES)],
         "g = 340 > N = 336: once every column is taken the rounds re-assign anchor 0 to ground truth 0",
         [("claimed", 1, 0, (0,))]),
]

_POS_UP, _NEG_UP = float(np.nextafter(0.5, 1)), float(np.nextafter(0.25, 1))
THRESHOLDS = [
    Case("thresholds_equal", [_gt([1] + TILES, [2] + LANES, [3] + FULL)],
         "IoU == pos_iou_threshold at 35 and 265 (matched), IoU == neg_iou_limit at 326, 329, 330 (neutral)",
         [("on_pos", 0, 0, (34, 35, 265)), ("on_neg", 0, 2, (325, 326, 329, 330))], breaks=SIZE_BREAKS),
    Case("pos_equal", [_gt([1] + TILES)], "IoU == pos_iou_threshold, neg_iou_limit out of reach",
         [("on_pos", 0, 0, (34, 35, 265))], breaks=SIZE_BREAKS, neg_iou_limit=0.75),
    Case("pos_next_up", [_gt([1] + TILES)], "the same box, pos_iou_threshold one float64 step higher: nothing but the bipartite match",
         [("only_bipartite", 0)], breaks=EXCLUDE_BREAKS, pos_iou_threshold=_POS_UP, neg_iou_limit=0.75),
    Case("neg_equal", [_gt([3] + FULL)], "IoU == neg_iou_limit", [("on_neg", 0, 0, (325, 326, 329, 330))], breaks=SIZE_BREAKS),
    Case("neg_next_up", [_gt([3] + FULL)], "the same box, neg_iou_limit one float64 step higher: nothing is neutral",
         [("only_bipartite", 0)], breaks=EXCLUDE_BREAKS, neg_iou_limit=_NEG_UP),
]


def _class_case(C, base=None):
    """B = 3 with every kind of row (matched by a tie, neutral, background), the highest class id in use, an empty image."""
    top = C - 1
    gt = [_gt([top] + TILES, [1] + LANES, [top] + FULL, [2] + FOUR), EMPTY,
          np.concatenate([random_boxes(12, top, 100 + C), _gt([top] + WAVES)], axis=0)]
    L, ta32, ta64 = CLASS_TABLE[C]
    name = "classes_%d" % C if base is None else "odd_n_classes_%d" % C
    return Case(name, gt, "L = %d: finalize_kernel<float> on tiles of %d anchors, <double> on %d" % (L, ta32, ta64), base=base, n_classes=top)


CLASSES = [_class_case(C) for C in CLASS_TABLE]
CLASSES_ODD_N = [_class_case(C, ODD_N) for C in CLASS_TABLE]        # N = 329: the store path test only

NAMED = TIES + QUIRKS + THRESHOLDS + CLASSES
GOLDEN = TIES + QUIRKS + THRESHOLDS                        # what tests/golden/encoder_edges.npz holds (make_golden.gen_encoder_edges)


@functools.lru_cache(maxsize=None)
def ladder(count):
    """One rung: the image with `count` boxes between an empty image and a one-box image, so that gt_off is (0, 0, count, count + 1)."""
    return Case("ladder_%d" % count, [EMPTY, random_boxes(count, 5, 1000 + count), _gt([2] + LANES)],
                "%d boxes: match_kernel LDS %d bytes" % (count, match_lds_bytes(count)), neg_iou_limit=0.3)


ALL_EMPTY = Case("all_empty", [EMPTY, EMPTY, EMPTY], "G_total == 0: the R and M kernels are skipped")
