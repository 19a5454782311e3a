#!/usr/bin/env python3
"""Generate the golden fixtures in this directory FROM THE REAL REFERENCE.

Run in the build container only (the reference is mounted at /root/reference there and
does not exist on the GPU box):

    python tests/golden/make_golden.py

It imports pierluigiferrari/ssd_keras's NumPy half unmodified (three removed NumPy aliases
are restored first), feeds it seeded inputs and stores inputs + outputs as .npz files.
`tests/test_oracle_golden.py` pins `oracle/np_oracle.py` to these files; the `-m gpu`
tests compare the HIP path with them.  The TensorFlow half of the reference (SSDLoss,
DecodeDetections layers, L2Normalization) cannot run here -> no goldens for it.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = os.environ.get("SSD_REFERENCE", "/root/reference")
sys.path.insert(0, REF)
np.float = float   # noqa: aliases removed in NumPy >= 1.24, used by the reference
np.int = int       # noqa
np.bool = bool     # noqa

from bounding_box_utils.bounding_box_utils import (convert_coordinates, convert_coordinates2, intersection_area,  # noqa: E402
                                                    iou)
from ssd_encoder_decoder.matching_utils import match_bipartite_greedy, match_multi     # noqa: E402
from ssd_encoder_decoder.ssd_input_encoder import SSDInputEncoder                      # noqa: E402
from ssd_encoder_decoder.ssd_output_decoder import (decode_detections, decode_detections_debug,  # noqa: E402
                                                    decode_detections_fast, greedy_nms, _greedy_nms, _greedy_nms2)

from ssd_keras_amd import synthetic as syn                                             # noqa: E402


def encoder_from(cfg, **over):
    kw = dict(cfg)
    kw.update(over)
    kw["predictor_sizes"] = np.array(kw["predictor_sizes"])
    return SSDInputEncoder(**kw)


def anchors_var(enc):
    t = enc.generate_encoding_template(batch_size=1)
    return t[0, :, -8:]


def ragged(list_of_arrays, width):
    rows = [np.asarray(a, dtype=np.float64).reshape(-1, width) for a in list_of_arrays]
    off = np.cumsum([0] + [r.shape[0] for r in rows]).astype(np.int64)
    return (np.concatenate(rows, axis=0) if rows else np.zeros((0, width))), off


def save(name, **arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("%-28s %8.1f KB  %d arrays" % (name, os.path.getsize(path) / 1024.0, len(arrays)))


# ----------------------------------------------------------------------------------------
def gen_box_utils():
    rng = np.random.RandomState(11)
    out = {}
    a = rng.uniform(0, 50, size=(7, 2))
    b = rng.uniform(0, 50, size=(9, 2))
    c1 = np.concatenate([a, a + rng.uniform(1, 40, size=(7, 2))], axis=1)   # corners
    c2 = np.concatenate([b, b + rng.uniform(1, 40, size=(9, 2))], axis=1)
    out["corners1"], out["corners2"] = c1, c2
    for conv in ("minmax2centroids", "centroids2minmax", "corners2centroids", "centroids2corners",
                 "minmax2corners", "corners2minmax"):
        for bp in ("half", "include", "exclude"):
            out["cc_%s_%s" % (conv, bp)] = convert_coordinates(c1, 0, conv, bp)
        out["cc32_%s" % conv] = convert_coordinates(c1.astype(np.float32), 0, conv, "half")
    for coords in ("corners", "minmax", "centroids"):
        if coords == "corners":
            p, q = c1, c2
        elif coords == "minmax":
            p, q = c1[:, [0, 2, 1, 3]], c2[:, [0, 2, 1, 3]]
        else:
            p, q = convert_coordinates(c1, 0, "corners2centroids"), convert_coordinates(c2, 0, "corners2centroids")
        for bp in ("half", "include", "exclude"):
            out["iou_outer_%s_%s" % (coords, bp)] = iou(p, q, coords, "outer_product", bp)
            out["iou_elem_%s_%s" % (coords, bp)] = iou(p, q[:7], coords, "element-wise", bp)
            out["iou_bcast_%s_%s" % (coords, bp)] = iou(p, q[3], coords, "element-wise", bp)
    # matching, including the zero-row / duplicate-anchor quirks
    mats = [np.array([[0, 0, 0, 0], [0, .6, 0, 0], [0, 0, 0, 0]], dtype=np.float64),
            np.array([[.5, .6], [0, 0]], dtype=np.float64),
            np.array([[.3, .3, .1], [.3, .3, .2]], dtype=np.float64),
            rng.uniform(0, 1, size=(5, 40)) * (rng.uniform(0, 1, size=(5, 40)) > 0.6),
            rng.uniform(0, 1, size=(8, 8))]
    for i, m in enumerate(mats):
        out["match_in_%d" % i] = m
        out["match_bip_%d" % i] = match_bipartite_greedy(m)
        g, a_ = match_multi(m, 0.5)
        out["match_multi_gt_%d" % i], out["match_multi_anchor_%d" % i] = g, a_
    save("box_utils", **out)


def gen_box_utils2():
    """Second box-utilities fixture: the public callables the first one does not cover (intersection_area, float32 /
    mixed-dtype iou, nD convert_coordinates, convert_coordinates2, the greedy_nms family in every coords format,
    larger / tie-heavy / signed matching problems)."""
    rng = np.random.RandomState(23)
    out = {}

    def boxes(n, lo=0.0, hi=60.0):
        a = rng.uniform(lo, hi, size=(n, 2))
        return np.concatenate([a, a + rng.uniform(1, 35, size=(n, 2))], axis=1)        # corners

    c1, c2 = boxes(13), boxes(17)
    out["corners1"], out["corners2"] = c1, c2
    views = {"corners": (c1, c2), "minmax": (c1[:, [0, 2, 1, 3]], c2[:, [0, 2, 1, 3]]),
             "centroids": (convert_coordinates(c1, 0, "corners2centroids"), convert_coordinates(c2, 0, "corners2centroids"))}
    for coords, (p, q) in views.items():
        for bp in ("half", "include", "exclude"):
            out["ia_outer_%s_%s" % (coords, bp)] = intersection_area(p, q, coords, "outer_product", bp)
            out["ia_elem_%s_%s" % (coords, bp)] = intersection_area(p, q[:13], coords, "element-wise", bp)
            # dtype rules: float32 x float32, float32 x float64
            p32, q32 = p.astype(np.float32), q.astype(np.float32)
            r = iou(p32, q32, coords, "outer_product", bp)
            out["iou32_outer_%s_%s" % (coords, bp)] = r
            out["iou32_outer_%s_%s_dtype" % (coords, bp)] = np.array(r.dtype.name)
            r = iou(p32, q, coords, "outer_product", bp)
            out["iou3264_outer_%s_%s" % (coords, bp)] = r
            r = iou(p, q32[:13], coords, "element-wise", bp)
            out["iou6432_elem_%s_%s" % (coords, bp)] = r
            r = intersection_area(p32, q32, coords, "outer_product", bp)
            out["ia32_outer_%s_%s" % (coords, bp)] = r
    # nD tensor, coordinates in the middle of the last axis
    t = rng.uniform(0, 40, size=(2, 5, 9))
    out["nd_in"] = t
    for conv in ("minmax2centroids", "centroids2minmax", "corners2centroids", "centroids2corners", "minmax2corners",
                 "corners2minmax"):
        out["nd_%s" % conv] = convert_coordinates(t, 3, conv, "include")
        out["nd32_%s" % conv] = convert_coordinates(t.astype(np.float32), 3, conv, "exclude")
    for conv in ("minmax2centroids", "centroids2minmax"):
        out["cc2_%s" % conv] = convert_coordinates2(t, 3, conv)
        out["cc2_32_%s" % conv] = convert_coordinates2(t.astype(np.float32), 3, conv)
    # greedy NMS family
    def table(n, lead, coords):
        b = boxes(n, 0, 40)
        if coords == "minmax":
            b = b[:, [0, 2, 1, 3]]
        elif coords == "centroids":
            b = convert_coordinates(b, 0, "corners2centroids")
        score = np.round(rng.uniform(0, 1, size=(n, 1)), 2)            # two decimals: plenty of ties
        cols = [rng.randint(1, 4, size=(n, 1)).astype(np.float64)] * (lead - 1) + [score, b]
        return np.concatenate(cols, axis=1)
    for coords in ("corners", "minmax", "centroids"):
        for bp in ("half", "include", "exclude"):
            items = [table(60, 2, coords), np.zeros((0, 6)), table(1, 2, coords), table(150, 2, coords)]
            cat, off = ragged(items, 6)
            res = greedy_nms(items, iou_threshold=0.45, coords=coords, border_pixels=bp)
            rcat, roff = ragged(res, 6)
            pre = "nms_%s_%s_" % (coords, bp)
            out[pre + "in"], out[pre + "in_off"], out[pre + "out"], out[pre + "out_off"] = cat, off, rcat, roff
    t5 = table(90, 1, "corners")
    out["nms1_in"], out["nms1_out"] = t5, _greedy_nms(t5, iou_threshold=0.3, coords="corners", border_pixels="half")
    t6 = table(90, 2, "corners")
    out["nms2_in"], out["nms2_out"] = t6, _greedy_nms2(t6, iou_threshold=0.6, coords="corners", border_pixels="include")
    # matching: larger, tie-heavy (quantised), sparse, and signed matrices
    mats = [np.round(rng.uniform(0, 1, size=(12, 300)), 1),
            rng.uniform(0, 1, size=(20, 700)) * (rng.uniform(0, 1, size=(20, 700)) > 0.97),
            rng.uniform(-1, 1, size=(6, 30)),
            -rng.uniform(0, 1, size=(4, 9)),
            np.zeros((3, 5)),
            rng.uniform(0, 1, size=(1, 1))]
    for i, m in enumerate(mats):
        out["match_in_%d" % i] = m
        out["match_bip_%d" % i] = match_bipartite_greedy(m)
        g, a_ = match_multi(m, 0.5)
        out["match_multi_gt_%d" % i], out["match_multi_anchor_%d" % i] = g, a_
    save("box_utils2", **out)


def _import_reference_evaluator():
    """The reference Evaluator imports its data generator (cv2 / h5py / PIL are absent here); stub those modules -- none of
    the methods pinned below touches them -- and import the real class."""
    import types
    for name, attrs in {"data_generator": [], "data_generator.object_detection_2d_data_generator": ["DataGenerator"],
                        "data_generator.object_detection_2d_geometric_ops": ["Resize"],
                        "data_generator.object_detection_2d_patch_sampling_ops": ["RandomPadFixedAR"],
                        "data_generator.object_detection_2d_photometric_ops": ["ConvertTo3Channels"],
                        "data_generator.object_detection_2d_misc_utils": ["apply_inverse_transforms"]}.items():
        if name not in sys.modules:
            m = types.ModuleType(name)
            for a in attrs:
                setattr(m, a, type(a, (), {}))
            sys.modules[name] = m
    from eval_utils.average_precision_evaluator import Evaluator
    return Evaluator


def make_eval_case(seed, n_images=40, n_classes=4, neutral=True, int_labels=True, empty_last_class=False):
    """Synthetic detection results + ground truth: jittered copies of the boxes (duplicates), random false positives,
    two-decimal confidences (plenty of ties), images without boxes, optional 'difficult' flags.  Labels are integer arrays, as
    the reference's dataset parsers produce them (get_num_gt_per_class indexes an array with the class id, :525)."""
    rng = np.random.RandomState(seed)
    labels, neutrals, image_ids = [], [], []
    preds = [[] for _ in range(n_classes + 1)]
    for i in range(n_images):
        image_ids.append("%06d" % (i * 7 + 3))
        g = int(rng.randint(0, 7)) if i % 9 else 0
        cls = rng.randint(1, n_classes + 1, size=g)
        x0 = rng.uniform(0, 200, size=g); y0 = rng.uniform(0, 200, size=g)
        w = rng.uniform(10, 90, size=g); h = rng.uniform(10, 90, size=g)
        lab = np.stack([cls.astype(np.float64), x0, y0, x0 + w, y0 + h], axis=1) if g else np.zeros((0, 5))
        if int_labels:
            lab = np.round(lab).astype(np.int64)
        labels.append(lab)
        neutrals.append(rng.uniform(size=g) < 0.25)
        for b in lab:
            for _ in range(int(rng.randint(0, 4))):                      # 0-3 detections per object -> duplicates
                jit = rng.normal(0, 6, size=4)
                c = int(b[0]) if rng.uniform() < 0.85 else int(rng.randint(1, n_classes + 1))
                preds[c].append((image_ids[-1], float(np.round(rng.uniform(0.02, 1.0), 2)), float(b[1] + jit[0]), float(b[2] + jit[1]),
                                 float(b[3] + jit[2]), float(b[4] + jit[3])))
        for _ in range(int(rng.randint(0, 5))):                          # background detections
            c = int(rng.randint(1, n_classes + 1))
            x, y = rng.uniform(0, 250, size=2)
            preds[c].append((image_ids[-1], float(np.round(rng.uniform(0.02, 0.6), 2)), float(x), float(y), float(x + rng.uniform(5, 60)),
                             float(y + rng.uniform(5, 60))))
    if empty_last_class:
        preds[n_classes] = []
    return labels, (neutrals if neutral else None), image_ids, preds


def gen_evaluator():
    import contextlib
    import io
    Evaluator = _import_reference_evaluator()
    out = {}
    cases = [dict(seed=1, neutral=True, ignore=True, thr=0.5, bp="include"), dict(seed=2, neutral=True, ignore=False, thr=0.5, bp="half"),
             dict(seed=3, neutral=False, ignore=True, thr=0.3, bp="exclude"), dict(seed=4, neutral=True, ignore=True, thr=0.75, bp="include"),
             # a class without predictions: the reference then leaves its cumulative lists one entry short (:616-620) and
             # compute_precision_recall raises IndexError -- only match_predictions is pinned for this case
             dict(seed=5, neutral=True, ignore=True, thr=0.5, bp="include", empty_last_class=True)]
    for ci, case in enumerate(cases):
        labels, neutrals, image_ids, preds = make_eval_case(case["seed"], neutral=case["neutral"], empty_last_class=case.get("empty_last_class", False))
        gen = type("Gen", (), {})()
        gen.labels, gen.eval_neutral, gen.image_ids = labels, neutrals, image_ids
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ev = Evaluator(model=None, n_classes=4, data_generator=gen)
        ev.prediction_results = preds
        sink = io.StringIO()
        with contextlib.redirect_stdout(sink), np.errstate(divide="ignore", invalid="ignore"):
            num_gt = ev.get_num_gt_per_class(ignore_neutral_boxes=case["ignore"], verbose=False, ret=True)
            tp, fp, ctp, cfp = ev.match_predictions(ignore_neutral_boxes=case["ignore"], matching_iou_threshold=case["thr"],
                                                    border_pixels=case["bp"], sorting_algorithm="mergesort", verbose=True, ret=True)
            if case.get("empty_last_class"):
                prec, rec, ap_s, ap_i, map_s, map_i = [[]], [[]], [0.0], [0.0], 0.0, 0.0
            else:
                prec, rec = ev.compute_precision_recall(verbose=False, ret=True)
                ap_s = ev.compute_average_precisions(mode="sample", num_recall_points=11, verbose=False, ret=True)
                map_s = ev.compute_mean_average_precision(ret=True)
                ap_i = ev.compute_average_precisions(mode="integrate", verbose=False, ret=True)
                map_i = ev.compute_mean_average_precision(ret=True)
        pre = "e%d_" % ci
        lab_cat, lab_off = ragged(labels, 5)
        out[pre + "labels"], out[pre + "labels_off"] = lab_cat, lab_off
        out[pre + "neutral"] = np.concatenate([np.asarray(n, dtype=np.uint8) for n in neutrals]) if neutrals is not None else np.zeros((0,), np.uint8)
        out[pre + "has_neutral"] = np.array(int(neutrals is not None))
        out[pre + "image_ids"] = np.array(image_ids)
        out[pre + "params"] = np.array(repr(case))
        out[pre + "num_gt"] = np.asarray(num_gt)
        for c in range(1, 5):
            pc = preds[c]
            out[pre + "c%d_pred_img" % c] = np.array([q[0] for q in pc]) if pc else np.zeros((0,), dtype="U6")
            out[pre + "c%d_pred" % c] = np.array([q[1:] for q in pc], dtype=np.float64).reshape(-1, 5)
            out[pre + "c%d_tp" % c], out[pre + "c%d_fp" % c] = np.asarray(tp[c]), np.asarray(fp[c])
            # classes without predictions get no cumulative / precision entries in the reference (:616-620 `continue`)
            if len(pc):
                out[pre + "c%d_ctp" % c], out[pre + "c%d_cfp" % c] = np.asarray(ctp[c]), np.asarray(cfp[c])
        out[pre + "ap_sample"], out[pre + "ap_integrate"] = np.asarray(ap_s, dtype=np.float64), np.asarray(ap_i, dtype=np.float64)
        out[pre + "map_sample"], out[pre + "map_integrate"] = np.array(map_s), np.array(map_i)
        out[pre + "n_prec"] = np.array(len(prec))
        for c in range(1, len(prec)):
            out[pre + "c%d_prec" % c], out[pre + "c%d_rec" % c] = np.asarray(prec[c], dtype=np.float64), np.asarray(rec[c], dtype=np.float64)
    out["n_cases"] = np.array(len(cases))
    save("evaluator", **out)


def gen_box_filter():
    """BoxFilter / ImageValidator of the real reference (data_generator/object_detection_2d_image_boxes_validation_utils.py).
    Stored compactly: the label sets once, per case the configuration, the indices of the rows the reference kept (its output
    preserves row order, so they are recovered by a sequential match) and the two ImageValidator verdicts."""
    from data_generator.object_detection_2d_image_boxes_validation_utils import BoxFilter, ImageValidator
    rng = np.random.RandomState(31)
    out = {}
    cfgs, kept_idx, kept_off, valid = [], [], [0], []
    sets = 0
    for dtype in (np.int64, np.float64):
        for trial in range(3):
            n = int(rng.randint(0, 14)) if trial else 12
            x0 = rng.uniform(-40, 260, size=n); y0 = rng.uniform(-40, 200, size=n)
            w = rng.uniform(-5, 120, size=n); h = rng.uniform(-5, 120, size=n)          # some degenerate / tiny boxes
            lab = np.stack([rng.randint(1, 21, size=n).astype(np.float64), x0, y0, x0 + w, y0 + h], axis=1)
            lab = np.round(lab).astype(np.int64) if dtype is np.int64 else lab
            H, W = int(rng.randint(100, 240)), int(rng.randint(120, 300))
            out["L%d" % sets], out["L%d_hw" % sets] = lab, np.array([H, W])
            for crit in ("center_point", "iou", "area"):
                for bp in ("half", "include", "exclude"):
                    for bounds in ((0.3, 1.0), (0.0, 1.0), (0.1, 0.6), (1.0, 1.0)):
                        for flags in ((True, True, True), (True, False, False), (False, True, True)):
                            f = BoxFilter(check_overlap=flags[0], check_min_area=flags[1], check_degenerate=flags[2], overlap_criterion=crit,
                                          overlap_bounds=bounds, min_area=16, border_pixels=bp)
                            with np.errstate(divide="ignore", invalid="ignore"):
                                kept = f(lab, H, W)
                            idx, j = [], 0
                            for row in kept:                                   # order-preserving subset -> indices
                                while not np.array_equal(lab[j], row):
                                    j += 1
                                idx.append(j)
                                j += 1
                            v = ImageValidator(overlap_criterion=crit, bounds=bounds, n_boxes_min=2, border_pixels=bp)
                            va = ImageValidator(overlap_criterion=crit, bounds=bounds, n_boxes_min="all", border_pixels=bp)
                            with np.errstate(divide="ignore", invalid="ignore"):
                                valid.append([bool(v(lab, H, W)), bool(va(lab, H, W))])
                            cfgs.append(repr(dict(set=sets, crit=crit, bp=bp, bounds=bounds, flags=flags)))
                            kept_idx += idx
                            kept_off.append(len(kept_idx))
            sets += 1
    out["cfgs"] = np.array(cfgs)
    out["kept_idx"], out["kept_off"] = np.array(kept_idx, dtype=np.int32), np.array(kept_off, dtype=np.int32)
    out["valid"] = np.array(valid, dtype=bool)
    out["n_sets"] = np.array(sets)
    save("box_filter", **out)


def gen_patch_sampling():
    """The reference's patch sampling ops (data_generator/object_detection_2d_patch_sampling_ops.py, NumPy only) and the box-level
    half of its original-SSD chain (SSDRandomCrop / SSDExpand of data_augmentation_chain_original_ssd.py; that module imports cv2
    for its photometric half, which is stubbed -- nothing pinned here calls it) on the seeded cases of tests/patch_cases.py."""
    import types
    if "cv2" not in sys.modules:
        class _Cv2Stub(types.ModuleType):
            def __getattr__(self, name):
                return 0
        sys.modules["cv2"] = _Cv2Stub("cv2")
    import data_generator.object_detection_2d_patch_sampling_ops as ops
    import data_generator.object_detection_2d_image_boxes_validation_utils as val
    import data_generator.data_augmentation_chain_original_ssd as chain
    from tests import patch_cases as pc
    ns = types.SimpleNamespace(SSDRandomCrop=chain.SSDRandomCrop, SSDExpand=chain.SSDExpand, BoundGenerator=val.BoundGenerator,
                               BoxFilter=val.BoxFilter, ImageValidator=val.ImageValidator)
    for name in ("PatchCoordinateGenerator", "CropPad", "Crop", "Pad", "RandomPatch", "RandomPatchInf", "RandomMaxCropFixedAR",
                 "RandomPadFixedAR"):
        setattr(ns, name, getattr(ops, name))
    out = {"n_cases": np.array(len(pc.CASES))}
    for i, case in enumerate(pc.CASES):
        res = pc.run(ns, case)
        for k, v in res.items():
            out["p%03d_%s" % (i, k)] = v
        out["p%03d_case" % i] = np.array(repr(case))
    save("patch_sampling", **out)


def gen_image_ops():
    """The reference's photometric ops, its resize / flip ops, SSDPhotometricDistortions and the whole SSDDataAugmentation chain
    (data_generator/object_detection_2d_photometric_ops.py, object_detection_2d_geometric_ops.py:27-262,
    data_augmentation_chain_original_ssd.py:146-280) on the seeded cases of tests/image_cases.py.  OpenCV is not installed: the
    modules run with a `cv2` built on oracle/np_image.py (cvtColor / LUT / equalizeHist / resize restated from OpenCV's published
    algorithms).  So these vectors pin everything the reference does AROUND those four primitives -- dtype round trips, NumPy
    arithmetic, clipping, in-place stores, random draws, label arithmetic, inverters, box filtering -- not the primitives."""
    import types
    from oracle import np_image as npi
    for name in [m for m in sys.modules if m == "cv2" or m.startswith("data_generator")]:
        del sys.modules[name]
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_RGB2HSV, cv2.COLOR_HSV2RGB, cv2.COLOR_RGB2GRAY = npi.COLOR_RGB2HSV, npi.COLOR_HSV2RGB, npi.COLOR_RGB2GRAY
    cv2.INTER_NEAREST, cv2.INTER_LINEAR, cv2.INTER_CUBIC, cv2.INTER_AREA, cv2.INTER_LANCZOS4 = 0, 1, 2, 3, 4
    cv2.BORDER_CONSTANT = 0
    cv2.cvtColor = lambda image, code: npi.cvt_color(np.ascontiguousarray(image), code)
    cv2.LUT = lambda image, table: npi.lut(image, table)
    cv2.equalizeHist = lambda plane: npi.equalize_hist(np.ascontiguousarray(plane))
    cv2.resize = lambda image, dsize=None, interpolation=1: npi.resize(np.ascontiguousarray(image), dsize, interpolation)
    sys.modules["cv2"] = cv2
    import data_generator.object_detection_2d_photometric_ops as pho
    import data_generator.object_detection_2d_geometric_ops as geo
    import data_generator.object_detection_2d_image_boxes_validation_utils as val
    import data_generator.data_augmentation_chain_original_ssd as chain
    from tests import image_cases as ic
    ns = types.SimpleNamespace(BoxFilter=val.BoxFilter, SSDPhotometricDistortions=chain.SSDPhotometricDistortions,
                               SSDDataAugmentation=chain.SSDDataAugmentation, Resize=geo.Resize, ResizeRandomInterp=geo.ResizeRandomInterp,
                               Flip=geo.Flip, RandomFlip=geo.RandomFlip)
    for name in ("ConvertColor", "ConvertDataType", "ConvertTo3Channels", "Hue", "RandomHue", "Saturation", "RandomSaturation", "Brightness",
                 "RandomBrightness", "Contrast", "RandomContrast", "HistogramEqualization", "RandomHistogramEqualization", "ChannelSwap",
                 "RandomChannelSwap"):
        setattr(ns, name, getattr(pho, name))
    out = {"n_cases": np.array(len(ic.CASES))}
    for i, case in enumerate(ic.CASES):
        res = ic.run(ns, case)
        for k, v in res.items():
            out["i%03d_%s" % (i, k)] = v
        out["i%03d_case" % i] = np.array(repr(case))
    # the call surface: constructor and __call__ signatures of every class the drop-in mirrors
    import inspect
    sigs = {}
    for name in sorted(vars(ns)):
        cls = getattr(ns, name)
        sigs[name] = (str(inspect.signature(cls.__init__)), str(inspect.signature(cls.__call__)))
    out["signatures"] = np.array(repr(sigs))
    save("image_ops", **out)
    for name in [m for m in sys.modules if m == "cv2" or m.startswith("data_generator")]:
        del sys.modules[name]


def gen_coco_utils():
    """The reference's eval_utils/coco_utils.predict_all_to_json (:62-200) on the seeded cases of tests/coco_cases.py: a stand-in
    generator / model around the REAL function, the real ConvertTo3Channels / RandomPadFixedAR / Resize (with the np_image-built cv2 of
    gen_image_ops: only Resize's pixels go through it, and no pixel reaches the results file) and, for model_mode='training', the real
    NumPy decode_detections.  Stored: the results file's text per case and how the function called the generator."""
    import tempfile
    import types
    from oracle import np_image as npi
    for name in [m for m in sys.modules if m == "cv2" or m.startswith("data_generator") or m.startswith("eval_utils")]:
        del sys.modules[name]
    cv2 = types.ModuleType("cv2")
    cv2.COLOR_RGB2HSV, cv2.COLOR_HSV2RGB, cv2.COLOR_RGB2GRAY = npi.COLOR_RGB2HSV, npi.COLOR_HSV2RGB, npi.COLOR_RGB2GRAY
    cv2.INTER_NEAREST, cv2.INTER_LINEAR, cv2.INTER_CUBIC, cv2.INTER_AREA, cv2.INTER_LANCZOS4 = 0, 1, 2, 3, 4
    cv2.BORDER_CONSTANT = 0
    cv2.cvtColor = lambda image, code: npi.cvt_color(np.ascontiguousarray(image), code)
    cv2.resize = lambda image, dsize=None, interpolation=1: npi.resize(np.ascontiguousarray(image), dsize, interpolation)
    sys.modules["cv2"] = cv2
    import eval_utils.coco_utils as ref_coco
    from tests import coco_cases as cc
    out = {"n_cases": np.array(len(cc.CASES))}
    with tempfile.TemporaryDirectory() as tmp:
        for i, case in enumerate(cc.CASES):
            res = cc.run(ref_coco, case, tmp)
            out["c%02d_json" % i] = np.array(res["json"])
            out["c%02d_error" % i] = np.array(res.get("error", ""))
            if res.get("error"):
                # the reference's 'pad' mode cannot run as written: :125 passes `clip_boxes`, which RandomPadFixedAR (:832) does not take;
                # and with THAT keyword dropped (what average_precision_evaluator.py:325 does) CropPad turns `labels=None` into a 0-d
                # array and indexes it (object_detection_2d_patch_sampling_ops.py:273, :325).  Both errors are recorded; the drop-in's
                # 'pad' mode works and is tested through a round-trip property instead (tests/test_coco_utils.py).
                real = ref_coco.RandomPadFixedAR
                ref_coco.RandomPadFixedAR = lambda patch_aspect_ratio, clip_boxes=False: real(patch_aspect_ratio=patch_aspect_ratio)
                try:
                    cc.run(ref_coco, case, tmp)
                    second = ""
                except Exception as exc:                          # noqa: BLE001
                    second = "%s: %s" % (type(exc).__name__, exc)
                finally:
                    ref_coco.RandomPadFixedAR = real
                out["c%02d_error_without_clip_boxes_kwarg" % i] = np.array(second)
            out["c%02d_generate_call" % i] = np.array(repr(res["generate_call"]))
            out["c%02d_batches_seen" % i] = np.array(repr(res["batches_seen"]))
            out["c%02d_case" % i] = np.array(repr(case))
        ann = os.path.join(tmp, "ann.json")
        import json
        cats = [{"id": cid, "name": nm, "supercategory": "x"} for cid, nm in ((1, "person"), (2, "bicycle"), (4, "motorcycle"), (7, "train"), (90, "toothbrush"))]
        with open(ann, "w") as f:
            json.dump({"categories": cats, "images": [], "annotations": []}, f)
        out["category_maps"] = np.array(repr(ref_coco.get_coco_category_maps(ann)))
        out["category_file"] = np.array(open(ann).read())
    save("coco_utils", **out)
    for name in [m for m in sys.modules if m == "cv2" or m.startswith("data_generator") or m.startswith("eval_utils")]:
        del sys.modules[name]


def gen_api_surface():
    """The reference's call surface read from its SOURCE with `ast` (tests/api_surface.py): parameter names, order
    and defaults of every callable the package mirrors -- including the TensorFlow / Keras modules that cannot be imported here."""
    from tests import api_surface
    import json
    out = api_surface.extract(REF)
    missing = [(m, q) for m, d in out.items() for q, v in d.items() if v is None]
    assert not missing, missing
    with open(os.path.join(HERE, "api_surface.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print("%-30s %6.1f KB" % ("api_surface.json", os.path.getsize(os.path.join(HERE, "api_surface.json")) / 1024.0))


def gen_anchors():
    out = {}
    for name, cfg in (("tiny", syn.TINY), ("ssd7", syn.SSD7_300), ("ssd300", syn.SSD300_VOC), ("ssd512", syn.SSD512_COCO)):
        for coords in ("centroids", "corners", "minmax"):
            for clip in (False, True):
                if name in ("ssd300", "ssd512") and (coords != "centroids" or clip):
                    continue
                enc = encoder_from(cfg, coords=coords, clip_boxes=clip)
                out["%s_%s_clip%d" % (name, coords, clip)] = np.concatenate([b.reshape(-1, 4) for b in enc.boxes_list])
    enc = encoder_from(syn.TINY, normalize_coords=False, steps=[8, (16, 20), 32, 64], offsets=[0.5, (0.3, 0.7), 0.5, 0.5])
    out["tiny_abs_steps"] = np.concatenate([b.reshape(-1, 4) for b in enc.boxes_list])
    save("anchors", **out)


def sparse_encoding(y, n_classes_incl_bg, background_id=0):
    """Rows of y_encoded that differ from the all-background template + checksums."""
    B = y.shape[0]
    touched = np.argwhere(y[:, :, background_id] != 1)
    # also rows whose offsets are non-zero (cannot happen for background rows, but be safe)
    extra = np.argwhere(np.any(y[:, :, -12:-8] != 0, axis=-1) & (y[:, :, background_id] == 1))
    idx = np.concatenate([touched, extra], axis=0) if extra.size else touched
    rows = y[idx[:, 0], idx[:, 1], :] if idx.size else np.zeros((0, y.shape[2]))
    return idx.astype(np.int32), rows, y.reshape(B, -1).sum(axis=1)


def gen_encoder():
    out = {}
    cases = []
    k = 0
    for coords in ("centroids", "corners", "minmax"):
        for matching in ("multi", "bipartite"):
            for bp, neg in (("half", 0.3), ("include", 0.5), ("exclude", 0.2)):
                cases.append(dict(cfg="tiny", coords=coords, matching_type=matching, border_pixels=bp,
                                  neg_iou_limit=neg, pos_iou_threshold=0.5, seed=100 + k, B=4, max_boxes=6))
                k += 1
    cases.append(dict(cfg="tiny", coords="centroids", matching_type="multi", border_pixels="half",
                      neg_iou_limit=0.3, pos_iou_threshold=0.5, seed=300, B=3, max_boxes=6, normalize_coords=False))
    cases.append(dict(cfg="tiny", coords="centroids", matching_type="multi", border_pixels="half",
                      neg_iou_limit=0.3, pos_iou_threshold=0.5, seed=301, B=3, max_boxes=6, background_id=2))
    cases.append(dict(cfg="ssd7", coords="centroids", matching_type="multi", border_pixels="half",
                      neg_iou_limit=0.3, pos_iou_threshold=0.5, seed=7, B=4, max_boxes=8))
    cases.append(dict(cfg="ssd300", coords="centroids", matching_type="multi", border_pixels="half",
                      neg_iou_limit=0.5, pos_iou_threshold=0.5, seed=7, B=4, max_boxes=8))
    cases.append(dict(cfg="ssd300", coords="centroids", matching_type="multi", border_pixels="half",
                      neg_iou_limit=0.3, pos_iou_threshold=0.5, seed=8, B=2, max_boxes=16, min_boxes=16))
    cfgs = dict(tiny=syn.TINY, ssd7=syn.SSD7_300, ssd300=syn.SSD300_VOC)
    for ci, case in enumerate(cases):
        cfg = cfgs[case["cfg"]]
        over = {k_: v for k_, v in case.items() if k_ not in ("cfg", "seed", "B", "max_boxes", "min_boxes")}
        enc = encoder_from(cfg, **over)
        gt = syn.make_ground_truth(case["B"], cfg["n_classes"], cfg["img_height"], cfg["img_width"],
                                   max_boxes=case["max_boxes"], seed=case["seed"], min_boxes=case.get("min_boxes", 1))
        if case["cfg"] == "tiny":
            # quirk coverage: an empty image, a far-away sliver that overlaps nothing, duplicates
            gt[1] = np.zeros((0, 5))
            gt[2] = np.concatenate([gt[2], [[1, 0.0, 0.0, 0.4, 0.4]], gt[2][:1]], axis=0)
        y, y_diag = enc(gt, diagnostics=True)
        idx, rows, sums = sparse_encoding(y, enc.n_classes, enc.background_id)
        gt_cat, gt_off = ragged(gt, 5)
        pre = "c%02d_" % ci
        out[pre + "gt"], out[pre + "gt_off"] = gt_cat, gt_off
        out[pre + "idx"], out[pre + "rows"], out[pre + "sums"] = idx, rows, sums
        out[pre + "diag_sums"] = y_diag.reshape(y.shape[0], -1).sum(axis=1)
        out[pre + "params"] = np.array(repr(case))
    out["n_cases"] = np.array(len(cases))
    save("encoder", **out)


def gen_encoder_edges():
    """The reference's encoder on the tie, threshold, quirk and g > N cases of tests/encode_cases.py (the dyadic configuration), for the
    three `coords` and both matching types: pins the ORACLE on the edges the device tests compare the kernels with it on.
    A few long arrays instead of several per run (an .npz member costs more than most of these results): the images of all cases
    in one ragged `gt`, `image_off` (cases + 1) into its images; run k = (case * 3 + coords) * 2 + matching owns
    idx / rows [run_off[k] : run_off[k + 1]] (sparse_encoding) and, per image, sums / diag_sums [image_run_off[k] : image_run_off[k + 1]]."""
    from tests import encode_cases as ec
    images, image_off, idx_all, rows_all, run_off, sums_all, diag_all, image_run_off = [], [0], [], [], [0], [], [], [0]
    for case in ec.GOLDEN:
        images += case.gt
        image_off.append(len(images))
        for coords in ec.COORDS:
            for matching in ec.MATCHING:
                enc = encoder_from(case.config(coords=coords, matching_type=matching))
                y, y_diag = enc([np.array(g) for g in case.gt], diagnostics=True)
                idx, rows, sums = sparse_encoding(y, enc.n_classes, enc.background_id)
                idx_all.append(idx.reshape(-1, 2))
                rows_all.append(rows)
                run_off.append(run_off[-1] + rows.shape[0])
                sums_all.append(sums)
                diag_all.append(y_diag.reshape(y.shape[0], -1).sum(axis=1))
                image_run_off.append(image_run_off[-1] + y.shape[0])
    gt_cat, gt_off = ragged(images, 5)
    save("encoder_edges", cases=np.array([c.name for c in ec.GOLDEN]), gt=gt_cat, gt_off=gt_off, image_off=np.array(image_off),
         idx=np.concatenate(idx_all).astype(np.int32), rows=np.concatenate(rows_all), run_off=np.array(run_off),
         sums=np.concatenate(sums_all), diag_sums=np.concatenate(diag_all), image_run_off=np.array(image_run_off))


def gen_decoder():
    out = {}
    cases = []
    # exp probe: lets a test tell whether the local np.exp(float32) is the one that made these files
    probe = np.linspace(-3, 3, 4001).astype(np.float32)
    out["exp_probe_in"], out["exp_probe_out"] = probe, np.exp(probe)

    def add(name, fn, y_pred, store_input, **kw):
        res = fn(y_pred, **kw)
        width = 7 if fn is decode_detections_debug else 6
        cat, off = ragged(res, width)
        pre = name + "_"
        out[pre + "out"], out[pre + "off"] = cat, off
        out[pre + "kw"] = np.array(repr(kw))
        out[pre + "fn"] = np.array(fn.__name__)
        if store_input is not None:
            out[pre + "y_pred"] = store_input
        cases.append(name)

    # --- TINY sweeps: every coords format / dtype / border mode --------------------------
    k = 0
    for coords in ("centroids", "corners", "minmax"):
        enc = encoder_from(syn.TINY, coords=coords)
        av = anchors_var(enc)
        for dtype in (np.float32, np.float64):
            for bias, thr in ((0.0, 0.05), (2.0, 0.01)):
                y = syn.make_y_pred(av, 3, enc.n_classes, bias=bias, seed=500 + k, dtype=dtype)
                tag = "tiny_%s_%s_b%d" % (coords, np.dtype(dtype).name, int(bias))
                out[tag + "_y_pred"] = y
                for bp in ("half", "include", "exclude"):
                    add("%s_%s" % (tag, bp), decode_detections, y, None, confidence_thresh=thr, iou_threshold=0.45,
                        top_k=200, input_coords=coords, normalize_coords=True, img_height=96, img_width=128,
                        border_pixels=bp)
                add(tag + "_top10", decode_detections, y, None, confidence_thresh=thr, iou_threshold=0.45, top_k=10,
                    input_coords=coords, normalize_coords=True, img_height=96, img_width=128)
                add(tag + "_all", decode_detections, y, None, confidence_thresh=thr, iou_threshold=0.3, top_k="all",
                    input_coords=coords, normalize_coords=False)
                add(tag + "_fast", decode_detections_fast, y, None, confidence_thresh=0.2, iou_threshold=0.45,
                    top_k="all", input_coords=coords, normalize_coords=True, img_height=96, img_width=128)
                add(tag + "_fast_top5", decode_detections_fast, y, None, confidence_thresh=0.1, iou_threshold=0.45,
                    top_k=5, input_coords=coords, normalize_coords=True, img_height=96, img_width=128)
                add(tag + "_fast_nonms", decode_detections_fast, y, None, confidence_thresh=0.3, iou_threshold=None,
                    top_k="all", input_coords=coords, normalize_coords=True, img_height=96, img_width=128)
                k += 1
    enc = encoder_from(syn.TINY)
    y = syn.make_y_pred(anchors_var(enc), 2, enc.n_classes, bias=1.0, seed=77)
    add("tiny_debug", decode_detections_debug, y, y, confidence_thresh=0.02, iou_threshold=0.45, top_k=50,
        input_coords="centroids", normalize_coords=True, img_height=96, img_width=128)
    add("tiny_debug_vit", decode_detections_debug, y, y, confidence_thresh=0.02, iou_threshold=0.45, top_k=50,
        input_coords="centroids", normalize_coords=True, img_height=96, img_width=128, variance_encoded_in_target=True)
    add("tiny_nothing", decode_detections, y, y, confidence_thresh=0.999, iou_threshold=0.45, top_k=200,
        input_coords="centroids", normalize_coords=True, img_height=96, img_width=128)

    # --- SSD7 dense (random-weights-like), SSD300 sparse (trained-like) --------------------
    enc = encoder_from(syn.SSD7_300)
    y = syn.make_y_pred(anchors_var(enc), 1, enc.n_classes, bias=0.0, seed=1234)
    out["ssd7_dense_conf_loc"] = y[:, :, :-8]
    add("ssd7_dense", decode_detections, y, None, confidence_thresh=0.01, iou_threshold=0.45, top_k=200,
        input_coords="centroids", normalize_coords=True, img_height=300, img_width=300)
    add("ssd7_dense_conf05", decode_detections, y, None, confidence_thresh=0.5, iou_threshold=0.45, top_k=200,
        input_coords="centroids", normalize_coords=True, img_height=300, img_width=300)
    enc = encoder_from(syn.SSD300_VOC)
    y = syn.make_y_pred(anchors_var(enc), 1, enc.n_classes, bias=7.0, seed=1234)
    out["ssd300_sparse_conf_loc"] = y[:, :, :-8]
    add("ssd300_sparse", decode_detections, y, None, confidence_thresh=0.01, iou_threshold=0.45, top_k=200,
        input_coords="centroids", normalize_coords=True, img_height=300, img_width=300)
    add("ssd300_sparse_include", decode_detections, y, None, confidence_thresh=0.01, iou_threshold=0.45, top_k=200,
        input_coords="centroids", normalize_coords=True, img_height=300, img_width=300, border_pixels="include")
    add("ssd300_fast", decode_detections_fast, y, None, confidence_thresh=0.1, iou_threshold=0.45, top_k=200,
        input_coords="centroids", normalize_coords=True, img_height=300, img_width=300)

    # --- public greedy_nms ------------------------------------------------------------------
    rng = np.random.RandomState(5)
    items = []
    for n in (0, 1, 37, 120):
        xy = rng.uniform(0, 80, size=(n, 2))
        box = np.concatenate([xy, xy + rng.uniform(5, 40, size=(n, 2))], axis=1)
        items.append(np.concatenate([rng.randint(1, 4, size=(n, 1)).astype(float), rng.uniform(size=(n, 1)), box], axis=1))
    cat, off = ragged(items, 6)
    out["gnms_in"], out["gnms_in_off"] = cat, off
    for bp in ("half", "include"):
        cat, off = ragged(greedy_nms([it for it in items if it.shape[0] > 0], 0.45, "corners", bp), 6)
        out["gnms_out_" + bp], out["gnms_out_off_" + bp] = cat, off
    out["cases"] = np.array(cases)
    save("decoder", **out)


if __name__ == "__main__":
    # box_filter / patch_sampling import the reference's real data_generator package; gen_evaluator stubs what is left of it
    gens = [gen_box_utils, gen_box_utils2, gen_box_filter, gen_patch_sampling, gen_image_ops, gen_coco_utils, gen_api_surface, gen_evaluator, gen_anchors, gen_encoder, gen_encoder_edges, gen_decoder]
    wanted = set(sys.argv[1:])
    for g in gens:
        if not wanted or g.__name__[4:] in wanted:
            g()
