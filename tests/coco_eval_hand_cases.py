"""COCO bbox evaluation cases small enough to work out on paper.  Every expectation below is a literal with its working in the
comment above it; tests/test_coco_eval_cpu.py holds the restatement (tests/np_cocoeval.py) to them, tests/test_coco_eval_gpu.py
the device evaluator.

Default parameters: IoU thresholds t = 0 .. 9 are 0.50, 0.55, ..., 0.95 (t = 5 is 0.75); area ranges a = 0 'all', 1 'small'
[0, 1024], 2 'medium' [1024, 9216], 3 'large' [9216, 1e10]; detection caps m = 0, 1, 2 are 1, 10, 100.
A case: images, categories (ids), gts, dts (result order; loadRes gives them id = position + 1), params (overrides) and `expect`:
    rows      (imgId, catId, a, t, dtMatches, dtIgnore)   one (area, threshold) row of a pair; matches are index + 1 into the
                                                          pair's ground truth in input order, 0 = unmatched
    gtIgnore  (imgId, catId, [A][G] flags)
    dtIds     (imgId, catId, ids in evaluation order)
    stats     the twelve numbers (to 1e-12)
    precision / recall   (index tuple, value) entries of the accumulated arrays; a slice(None) stands for a whole axis
"""

ONE_MINUS = 1.0 - 2.220446049250313e-16        # 1 / (0 + 1 + np.spacing(1)): the precision of a lone true positive


def _gt(id_, img, cat, bbox, area=None, iscrowd=0):
    return dict(id=id_, image_id=img, category_id=cat, bbox=list(bbox), area=bbox[2] * bbox[3] if area is None else area, iscrowd=iscrowd)


def _dt(img, cat, bbox, score):
    return dict(image_id=img, category_id=cat, bbox=list(bbox), score=score)


def _case(name, images, categories, gts, dts, expect, params=None):
    dts = [dict(d, id=i + 1) for i, d in enumerate(dts)]
    return dict(name=name, images=images, categories=categories, gts=gts, dts=dts, expect=expect, params=params or {})


F, T = False, True
ALL = slice(None)

CASES = []

# (a) IoU exactly on a threshold.
# image 1: gt [0,0,10,10] (100), dt [0,0,10,5] (50): w = 10, h = 5, i = 50, u = 50 + 100 - 50 = 100, IoU = 0.5 exactly: the walk starts
#   with best = 0.5 and skips only IoU < best, so it matches at t = 0 (0.50) and not at t = 1 (0.55).
# image 2: gt [0,0,16,16] (256), dt [0,0,16,12] (192): i = 192, u = 192 + 256 - 192 = 256, IoU = 0.75 exactly: matches at t = 5, not t = 6.
# 'medium' (a = 2): both ground truths are ignored (area < 1024); the matched detection inherits the flag, the unmatched one is
#   ignored because its own area (50, 192) is outside the range.
CASES.append(_case(
    "a_iou_on_threshold", [1, 2], [1],
    [_gt(1, 1, 1, [0, 0, 10, 10]), _gt(2, 2, 1, [0, 0, 16, 16])],
    [_dt(1, 1, [0, 0, 10, 5], 0.9), _dt(2, 1, [0, 0, 16, 12], 0.8)],
    dict(rows=[(1, 1, 0, 0, [1], [F]), (1, 1, 0, 1, [0], [F]), (2, 1, 0, 5, [1], [F]), (2, 1, 0, 6, [0], [F]),
               (1, 1, 2, 0, [1], [T]), (1, 1, 2, 1, [0], [T])],
         gtIgnore=[(1, 1, [[F], [F], [T], [T]])])))

# (b) Two ground truths of equal IoU: the comparison `IoU < best` is strict, so the later one replaces the earlier.
# gt 1 = gt 2 = [0,0,10,10]; dt 1 and dt 2 = [0,0,10,5]: IoU 0.5 with both.  t = 0: dt 1 (higher score) takes gt 2, dt 2 then finds gt 2
#   matched and takes gt 1.  t = 1: 0.5 < 0.55, nothing matches.
CASES.append(_case(
    "b_equal_iou_later_wins", [1], [1],
    [_gt(1, 1, 1, [0, 0, 10, 10]), _gt(2, 1, 1, [0, 0, 10, 10])],
    [_dt(1, 1, [0, 0, 10, 5], 0.9), _dt(1, 1, [0, 0, 10, 5], 0.8)],
    dict(rows=[(1, 1, 0, 0, [2, 1], [F, F]), (1, 1, 0, 1, [0, 0], [F, F])])))

# (c) A crowd ground truth matched by two detections.
# gt 1 crowd [0,0,20,20]; gt 2 [100,100,10,10].  Detections by score: A [0,0,10,10] and B [5,5,10,10] lie inside the crowd: i = 100,
#   u = da = 100, IoU = 1; C [15,15,10,10]: w = h = 20 - 15 = 5, i = 25, u = da = 100, IoU 0.25: unmatched; D = gt 2's box, IoU 1.
#   Sorted ground truth: gt 2 (not ignored), gt 1 (crowd = ignored).  A: gt 2 IoU 0, crowd IoU 1 -> crowd.  B: the crowd is matched
#   already but a crowd may be matched again -> crowd.  D: gt 2, then stops at the ignored crowd.  Row: matches [1, 1, 0, 2],
#   ignore [T, T, F, F] at every threshold (all IoUs are 1 or below 0.5).
#   Accumulate ('all', cap 100): npig = 1; tp = [0,0,0,1], fp = [0,0,1,1]; pr = [0,0,0,1/2]; envelope 1/2 everywhere; rc = [0,0,0,1]:
#   every recall threshold reads 1/2.  AP = 0.5.  All areas (100, 400) are 'small': medium / large have no ground truth: -1.
#   Cap 1 keeps only A (ignored): recall 0.  Caps 10, 100: recall 1.
CASES.append(_case(
    "c_crowd_matched_twice", [1], [1],
    [_gt(1, 1, 1, [0, 0, 20, 20], iscrowd=1), _gt(2, 1, 1, [100, 100, 10, 10])],
    [_dt(1, 1, [0, 0, 10, 10], 0.9), _dt(1, 1, [5, 5, 10, 10], 0.8), _dt(1, 1, [15, 15, 10, 10], 0.7), _dt(1, 1, [100, 100, 10, 10], 0.6)],
    dict(rows=[(1, 1, 0, 0, [1, 1, 0, 2], [T, T, F, F]), (1, 1, 0, 9, [1, 1, 0, 2], [T, T, F, F])],
         gtIgnore=[(1, 1, [[T, F], [T, F], [T, T], [T, T]])],
         stats=[0.5, 0.5, 0.5, 0.5, -1, -1, 0.0, 1.0, 1.0, 1.0, -1, -1])))

# (d) A detection preferring the non-ignored ground truth (the stop rule).
# gt 1 box [0,0,20,10], area field 500 (small); gt 2 box [0,0,20,20], area field 5000 (medium).  dt [0,0,20,16] (320):
#   with gt 1: i = 20 * 10 = 200, u = 320 + 200 - 200 = 320, IoU 0.625; with gt 2: i = 320, u = 320 + 400 - 320 = 400, IoU 0.8.
#   'all': neither is ignored, order gt 1, gt 2: 0.625 then 0.8 replaces it -> gt 2.
#   'small': gt 2 is ignored and sorts last.  t = 0: gt 1 (0.625 >= 0.5) is held, the walk stops at the ignored gt 2 -> gt 1, not ignored.
#            t = 3 (0.65): gt 1 fails, nothing is held, gt 2 (0.8) matches -> ignored.
#   'medium': gt 1 is ignored; order gt 2, gt 1: gt 2 is held, stop -> gt 2, not ignored.
CASES.append(_case(
    "d_stop_at_ignored", [1], [1],
    [_gt(1, 1, 1, [0, 0, 20, 10], area=500), _gt(2, 1, 1, [0, 0, 20, 20], area=5000)],
    [_dt(1, 1, [0, 0, 20, 16], 0.9)],
    dict(rows=[(1, 1, 0, 0, [2], [F]), (1, 1, 1, 0, [1], [F]), (1, 1, 1, 3, [2], [T]), (1, 1, 2, 0, [2], [F])],
         gtIgnore=[(1, 1, [[F, F], [F, T], [T, F], [T, T]])])))

# (e) The ground truth's `area` field decides its range, not its box: box 40 x 40 = 1600 ('medium') with area = 900 ('small').
#   The detection [0,0,40,40] (1600) matches it: in 'small' the ground truth counts and the matched detection is NOT ignored although
#   its own area is outside the range; in 'medium' the ground truth is ignored and so is the detection.
CASES.append(_case(
    "e_area_field", [1], [1],
    [_gt(1, 1, 1, [0, 0, 40, 40], area=900)],
    [_dt(1, 1, [0, 0, 40, 40], 0.9)],
    dict(rows=[(1, 1, 1, 0, [1], [F]), (1, 1, 2, 0, [1], [T]), (1, 1, 3, 0, [1], [T])],
         gtIgnore=[(1, 1, [[F], [F], [T], [T]])],
         stats=[ONE_MINUS, ONE_MINUS, ONE_MINUS, ONE_MINUS, -1, -1, 1.0, 1.0, 1.0, 1.0, -1, -1])))

# (f) Detection area against match status.
# gt 1 [0,0,40,40] area 1600 (medium); gt 2 [100,100,40,40] with area field 900 (small).  Detections: A = gt 1's box (1600), B
#   [200,200,10,10] (100, touches nothing), C = gt 2's box (1600).  Matches are [1, 0, 2] in every range (IoU 1 or 0).
#   'all':    nothing ignored.
#   'small':  gt 1 ignored.  A matched an ignored box: ignored.  B unmatched, 100 is inside [0, 1024]: not ignored.  C matched a
#             counted box: not ignored although 1600 is outside.
#   'medium': gt 2 ignored.  A not ignored.  B unmatched and 100 < 1024: ignored.  C matched an ignored box: ignored.
#   'large':  both ignored; B unmatched and 100 < 9216: ignored.
CASES.append(_case(
    "f_detection_area", [1], [1],
    [_gt(1, 1, 1, [0, 0, 40, 40]), _gt(2, 1, 1, [100, 100, 40, 40], area=900)],
    [_dt(1, 1, [0, 0, 40, 40], 0.9), _dt(1, 1, [200, 200, 10, 10], 0.8), _dt(1, 1, [100, 100, 40, 40], 0.7)],
    dict(rows=[(1, 1, 0, 0, [1, 0, 2], [F, F, F]), (1, 1, 1, 0, [1, 0, 2], [T, F, F]), (1, 1, 2, 0, [1, 0, 2], [F, T, T]),
               (1, 1, 3, 0, [1, 0, 2], [T, T, T])],
         gtIgnore=[(1, 1, [[F, F], [T, F], [F, T], [T, T]])])))

# (g) More than 100 detections in one pair, tied scores across the cut.
# 99 detections of score 0.9 far from the ground truth, then two of score 0.5: the first far away, the second exactly on the ground
#   truth.  The stable order keeps input order among equal scores, so the cut to 100 keeps ids 1 .. 100 and drops the only detection
#   that would match: no match anywhere, recall 0, precision 0.
CASES.append(_case(
    "g_cut_at_100_is_stable", [1], [1],
    [_gt(1, 1, 1, [0, 0, 10, 10])],
    [_dt(1, 1, [1000 + 10 * i, 0, 5, 5], 0.9) for i in range(99)] + [_dt(1, 1, [5000, 0, 5, 5], 0.5), _dt(1, 1, [0, 0, 10, 10], 0.5)],
    dict(rows=[(1, 1, 0, 0, [0] * 100, [F] * 100)],
         dtIds=[(1, 1, list(range(1, 101)))],
         stats=[0.0, 0.0, 0.0, 0.0, -1, -1, 0.0, 0.0, 0.0, 0.0, -1, -1])))

# (h) tp, fp, tp.  Two ground truths, detections A (on gt 1, 0.9), B (nowhere, 0.8), C (on gt 2, 0.7); IoUs are 1, so every threshold
#   agrees.  tp = [1,1,2], fp = [0,1,1], npig = 2: rc = [.5, .5, 1]; pr = [1/(1 + eps), 1/2, 2/3]; envelope [1 - 2.2e-16, 2/3, 2/3].
#   Recall thresholds 0 .. 0.5 (51 of them; recThrs[50] == 0.5 exactly) read position 0, the other 50 read position 2:
#   AP = (51 * (1 - 2.2e-16) + 50 * 2/3) / 101 = 253/303 - 1.1e-16 = 0.834983498349835.  Cap 1 keeps A: recall 0.5.
AP_H = 0.834983498349835
CASES.append(_case(
    "h_tp_fp_tp", [1], [1],
    [_gt(1, 1, 1, [0, 0, 10, 10]), _gt(2, 1, 1, [100, 0, 10, 10])],
    [_dt(1, 1, [0, 0, 10, 10], 0.9), _dt(1, 1, [50, 50, 10, 10], 0.8), _dt(1, 1, [100, 0, 10, 10], 0.7)],
    dict(rows=[(1, 1, 0, 0, [1, 0, 2], [F, F, F])],
         precision=[((0, 0, 0, 0, 2), ONE_MINUS), ((0, 50, 0, 0, 2), ONE_MINUS), ((0, 51, 0, 0, 2), 2.0 / 3.0), ((9, 100, 0, 0, 2), 2.0 / 3.0)],
         recall=[((0, 0, 0, 0), 0.5), ((0, 0, 0, 2), 1.0)],
         stats=[AP_H, AP_H, AP_H, AP_H, -1, -1, 0.5, 1.0, 1.0, 1.0, -1, -1])))

SUMMARY_H = [
    " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 0.835",
    " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = 0.835",
    " Average Precision  (AP) @[ IoU=0.75      | area=   all | maxDets=100 ] = 0.835",
    " Average Precision  (AP) @[ IoU=0.50:0.95 | area= small | maxDets=100 ] = 0.835",
    " Average Precision  (AP) @[ IoU=0.50:0.95 | area=medium | maxDets=100 ] = -1.000",
    " Average Precision  (AP) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = -1.000",
    " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = 0.500",
    " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets= 10 ] = 1.000",
    " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = 1.000",
    " Average Recall     (AR) @[ IoU=0.50:0.95 | area= small | maxDets=100 ] = 1.000",
    " Average Recall     (AR) @[ IoU=0.50:0.95 | area=medium | maxDets=100 ] = -1.000",
    " Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = -1.000",
]

# (i) The three empty sides.  Category 1: ground truth, no detections: precision 0 at every recall threshold, recall 0.  Category 2:
#   detections, no ground truth: npig = 0, everything stays -1.  Category 3: neither: -1.  The means skip the -1 entries: 0.
CASES.append(_case(
    "i_empty_sides", [1], [1, 2, 3],
    [_gt(1, 1, 1, [0, 0, 10, 10])],
    [_dt(1, 2, [0, 0, 10, 10], 0.9)],
    dict(precision=[((ALL, ALL, 0, 0, ALL), 0.0), ((ALL, ALL, 1, ALL, ALL), -1.0), ((ALL, ALL, 2, ALL, ALL), -1.0)],
         recall=[((ALL, 0, 0, ALL), 0.0), ((ALL, 1, ALL, ALL), -1.0), ((ALL, 2, ALL, ALL), -1.0)],
         stats=[0.0, 0.0, 0.0, 0.0, -1, -1, 0.0, 0.0, 0.0, 0.0, -1, -1])))

# (j) useCats.  A category-1 ground truth and a category-2 detection on the same box.  Per category nothing matches (AP 0, as in (i));
#   pooled into one category the detection is a true positive: precision 1 / (1 + eps) everywhere, recall 1.
CASES.append(_case(
    "j_use_cats_1", [1], [1, 2],
    [_gt(1, 1, 1, [0, 0, 10, 10])],
    [_dt(1, 2, [0, 0, 10, 10], 0.9)],
    dict(rows=[(1, 2, 0, 0, [0], [F])],
         stats=[0.0, 0.0, 0.0, 0.0, -1, -1, 0.0, 0.0, 0.0, 0.0, -1, -1])))
CASES.append(_case(
    "j_use_cats_0", [1], [1, 2],
    [_gt(1, 1, 1, [0, 0, 10, 10])],
    [_dt(1, 2, [0, 0, 10, 10], 0.9)],
    dict(rows=[(1, None, 0, 0, [1], [F]), (1, None, 0, 9, [1], [F])],
         stats=[ONE_MINUS, ONE_MINUS, ONE_MINUS, ONE_MINUS, -1, -1, 1.0, 1.0, 1.0, 1.0, -1, -1]),
    params=dict(useCats=0)))


def dataset(case):
    """The case's ground truth as a COCO annotation dict."""
    return dict(images=[dict(id=i) for i in case["images"]], categories=[dict(id=c, name="c%d" % c) for c in case["categories"]],
                annotations=[dict(g) for g in case["gts"]])


def check(case, matches, precision, recall, stats):
    """Hold one evaluation of `case` to its literals: `matches(imgId, catId)` returns a pair's arrays, the rest are the accumulated
    arrays and the twelve statistics.  Matches and flags exactly, numbers to 1e-12."""
    import numpy as np
    e = case["expect"]
    for img, cat, a, t, want_m, want_i in e.get("rows", []):
        got = matches(img, cat)
        assert got["dtMatches"][a, t].tolist() == want_m, (case["name"], img, cat, a, t, got["dtMatches"][a, t].tolist())
        assert got["dtIgnore"][a, t].tolist() == want_i, (case["name"], img, cat, a, t, got["dtIgnore"][a, t].tolist())
    for img, cat, want in e.get("gtIgnore", []):
        assert matches(img, cat)["gtIgnore"].tolist() == want, (case["name"], img, cat)
    for img, cat, want in e.get("dtIds", []):
        assert matches(img, cat)["dtIds"].tolist() == want, (case["name"], img, cat)
    for name, arr in (("precision", precision), ("recall", recall)):
        for idx, want in e.get(name, []):
            got = np.asarray(arr[idx])
            assert got.size > 0 and np.all(np.abs(got - want) <= 1e-12), (case["name"], name, idx, got)
    if "stats" in e:
        assert np.all(np.abs(np.asarray(stats) - np.asarray(e["stats"], dtype=np.float64)) <= 1e-12), (case["name"], list(stats))
