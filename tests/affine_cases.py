"""Seeded cases for Translate / Scale / Rotate and their random forms (data_generator/object_detection_2d_geometric_ops.py:233-772) and
the constant-input-size, variable-input-size and satellite chains.  The same builder runs against the reference's classes
(tests/golden/make_affine_golden.py, with a cv2 stub built on oracle/np_image.py and tests/np_warp.py) and against the drop-in's
(tests/test_affine_ops_cpu.py, tests/test_affine_ops_gpu.py): `ns` is any object carrying the class names used below.  Every case records
the output image, the labels and where both random generators (np.random and Python's random) stand afterwards."""
import hashlib
import random

import numpy as np

from tests.patch_cases import make_inputs

OPS = ("Translate", "RandomTranslate", "Scale", "RandomScale", "Rotate", "RandomRotate")
CHAINS = ("DataAugmentationConstantInputSize", "DataAugmentationVariableInputSize", "DataAugmentationSatellite")


def _cases():
    cases = []
    k = 0
    for labels in ("int", "float", None):
        for bf in (False, True):
            for clip in (True, False):
                for dy, dx in ((0.2, -0.15), (-0.37, 0.5)):
                    cases.append(dict(op="Translate", seed=k, labels=labels, box_filter=bf, clip_boxes=clip, dy=dy, dx=dx)); k += 1
                for factor in (0.6, 1.37):
                    cases.append(dict(op="Scale", seed=k, labels=labels, box_filter=bf, clip_boxes=clip, factor=factor)); k += 1
        for angle in (90, 180, 270):
            cases.append(dict(op="Rotate", seed=k, labels=labels, angle=angle, size=(20, 24) if angle != 180 else (17, 31))); k += 1
    for labels in ("int", "float", None):
        for validator in (False, True):
            for prob, n_trials in ((1.0, 3), (0.5, 1), (1.0, 0)):
                for op in ("RandomTranslate", "RandomScale"):
                    cases.append(dict(op=op, seed=k, labels=labels, box_filter=validator, validator=validator, clip_boxes=True, prob=prob,
                                      n_trials_max=n_trials)); k += 1
        for prob in (1.0, 0.5, 0.5):
            cases.append(dict(op="RandomRotate", seed=k, labels=labels, prob=prob)); k += 1
    for chain in CHAINS:
        for s in range(10):
            cases.append(dict(op=chain, seed=700 + 20 * CHAINS.index(chain) + s, labels=None if (chain == CHAINS[0] and s == 9) else "int",
                              n_boxes=1 + s % 4)); k += 1
    return cases


CASES = _cases()


def _box_filter(ns):
    return ns.BoxFilter(check_overlap=True, check_min_area=True, check_degenerate=True, overlap_criterion='area', overlap_bounds=(0.3, 1.0),
                        min_area=16)


def _validator(ns):
    return ns.ImageValidator(overlap_criterion='area', bounds=(0.5, 1.0), n_boxes_min=1)


def needs_boxes_kernel(case):
    """Cases whose host logic calls BoxFilter / ImageValidator (GPU kernels in the drop-in)."""
    return bool(case.get("box_filter") or case.get("validator")) or case["op"] in CHAINS


def run(ns, case):
    op = case["op"]
    np.random.seed(case["seed"])
    random.seed(case["seed"])
    size = case.get("size", (40, 48) if op in CHAINS else (20, 24))
    img, labels = make_inputs(case["seed"], case.get("n_boxes", 3), float_labels=case["labels"] == "float", size=size)
    if case["labels"] is None:
        labels = None
    if op == "Translate":
        t = ns.Translate(dy=case["dy"], dx=case["dx"], clip_boxes=case["clip_boxes"], box_filter=_box_filter(ns) if case["box_filter"] else None,
                         background=(10, 200, 30))
    elif op == "Scale":
        t = ns.Scale(factor=case["factor"], clip_boxes=case["clip_boxes"], box_filter=_box_filter(ns) if case["box_filter"] else None,
                     background=(255, 0, 77))
    elif op == "Rotate":
        t = ns.Rotate(angle=case["angle"])
    elif op == "RandomTranslate":
        t = ns.RandomTranslate(dy_minmax=(0.03, 0.5), dx_minmax=(0.03, 0.5), prob=case["prob"], clip_boxes=case["clip_boxes"],
                               box_filter=_box_filter(ns) if case["box_filter"] else None,
                               image_validator=_validator(ns) if case["validator"] else None, n_trials_max=case["n_trials_max"],
                               background=(1, 2, 3))
    elif op == "RandomScale":
        t = ns.RandomScale(min_factor=0.5, max_factor=2.0, prob=case["prob"], clip_boxes=case["clip_boxes"],
                           box_filter=_box_filter(ns) if case["box_filter"] else None,
                           image_validator=_validator(ns) if case["validator"] else None, n_trials_max=case["n_trials_max"],
                           background=(9, 8, 7))
    elif op == "RandomRotate":
        t = ns.RandomRotate(prob=case["prob"])
    elif op == "DataAugmentationConstantInputSize":
        t = ns.DataAugmentationConstantInputSize()
    elif op in ("DataAugmentationVariableInputSize", "DataAugmentationSatellite"):
        t = getattr(ns, op)(resize_height=30, resize_width=36)
    else:
        raise ValueError(op)
    out = {}
    if labels is None:
        res = t(img)
    else:
        res, lab = t(img, labels)
        lab = np.asarray(lab)
        out["labels"] = lab
        out["labels_dtype"] = np.array(str(lab.dtype))
    out["image"] = np.ascontiguousarray(res)
    out["np_state"], out["py_state"] = generator_digests()
    return out


def generator_digests():
    """SHA-256 of the whole state of np.random (624 key words + position) and of Python's random (625 words): equal digests = equal
    states, at 64 bytes per case instead of 5 KB."""
    key, pos = np.random.get_state()[1:3]
    np_words = np.append(np.asarray(key, dtype=np.uint32), np.uint32(pos))
    py_words = np.asarray(random.getstate()[1], dtype=np.uint32)
    return (np.array(hashlib.sha256(np_words.astype("<u4").tobytes()).hexdigest()),
            np.array(hashlib.sha256(py_words.astype("<u4").tobytes()).hexdigest()))
