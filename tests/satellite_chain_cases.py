"""What tests/test_satellite_chain_device_cpu.py and tests/test_satellite_chain_device_gpu.py share: the chain's constructor, ragged
batches of small images, the per-image reference (`np.random.seed(s); random.seed(s); chain(image, labels)`), a trace of what the
chain's OWN host ops did to each image (the branch table is asserted from it, never from the code under test), the golden satellite
cases of tests/golden/affine_ops.npz, and NumPy stand-ins for the kernels so that the host logic runs without a GPU."""
import hashlib
import random

import numpy as np

from tests import affine_cases as ac
from tests import np_satellite_chain as nsc
from tests import util
from tests import variable_chain_cases as vc
from tests.patch_cases import make_inputs

OUT = (30, 36)
SIZES = vc.SIZES                  # (H, W) between 24 x 40 and 96 x 128: landscape, portrait, square and odd sizes
# per-image seeds (np.random.seed(s); random.seed(s)) under which the default configuration on `batch()` takes every branch of the table,
# and one seed for both generators in front of `batch()` walked as ONE stream with the same coverage -- found on the CPU with the NumPy
# stand-ins below; the tests assert the branches from the host loop's trace
BRANCH_SEEDS = [1088, 1047, 1001, 1005, 1000, 1000, 1000, 1000]
BRANCH_STREAM_SEED = 68
# a stream seed under which at least three images of `batch()` rotate, by all three angles (Python's generator advances by that many
# draws)
ROTATING_STREAM_SEED = 0

state_row, same_state, assert_equal = vc.state_row, vc.same_state, vc.assert_equal


def chain(out=OUT, **kw):
    from ssd_keras_amd.data_generator.data_augmentation_chain_satellite import DataAugmentationSatellite
    return DataAugmentationSatellite(resize_height=out[0], resize_width=out[1], **kw)


def batch(B=8, seed=7, sizes=SIZES):
    return vc.batch(B, seed, sizes)


def seed_both(s):
    np.random.seed(s)
    random.seed(s)


def per_image(ch, images, labels, seeds):
    """[(pixels, labels, np.random state (625,))] of `np.random.seed(s); random.seed(s); chain(image, labels)`; both global generators
    are put back."""
    saved, saved_py, out = np.random.get_state(), random.getstate(), []
    try:
        for img, lab, s in zip(images, labels, seeds):
            seed_both(s)
            px, lb = ch(img, lab)
            out.append((px, lb, state_row(np.random.get_state())))
    finally:
        np.random.set_state(saved)
        random.setstate(saved_py)
    return out


def call_loop(ch, images, labels):
    """[(pixels, labels, None)] of `for i: chain(image_i, labels_i)` on the global generators (which move)."""
    return [ch(img, lab) + (None,) for img, lab in zip(images, labels)]


def trace(ch, shapes, labels, seeds=None):
    """What the chain's own host ops do to each image, observed on lazy images (no pixels): which flips ran, the rotation's angle (0 =
    none), the patch (top, left, h, w) on the rotated image or None and its kind, the trial that was accepted, boxes the patch filter
    removed, boxes min_area removed behind the resize, boxes left.  `seeds`: one per image for both generators, else the global
    streams go on from image to image; both are put back."""
    from ssd_keras_amd.data_generator import _image_ops as iop
    from ssd_keras_amd.data_generator.object_detection_2d_geometric_ops import Flip, Rotate
    from ssd_keras_amd.data_generator.object_detection_2d_image_boxes_validation_utils import ImageValidator
    from ssd_keras_amd.data_generator.object_detection_2d_patch_sampling_ops import CropPad
    real_cut, real_flip, real_rotate, real_validate = CropPad.__call__, Flip.__call__, Rotate.__call__, ImageValidator.validate_patches
    seen = {}

    def cut(self, image, labels=None, return_inverter=False):
        out = real_cut(self, image, labels, return_inverter)
        seen["patch"] = (self.patch_ymin, self.patch_xmin, self.patch_height, self.patch_width)
        seen["patch_dropped"] = len(labels) - len(out[1])
        return out

    def flip(self, image, labels=None, return_inverter=False):
        seen[self.dim] = True
        return real_flip(self, image, labels, return_inverter)

    def rotate(self, image, labels=None):
        seen["angle"] = int(self.angle)
        return real_rotate(self, image, labels)

    def validate(self, labels, ys, xs, hs, ws):
        valid = real_validate(self, labels, ys, xs, hs, ws)
        hits = np.flatnonzero(valid)
        seen["trial"] = int(hits[0]) + 1 if hits.size else 0
        return valid

    saved, saved_py, rows = np.random.get_state(), random.getstate(), []
    CropPad.__call__, Flip.__call__, Rotate.__call__, ImageValidator.validate_patches = cut, flip, rotate, validate
    try:
        ch._sync_formats()
        lf = ch.labels_format
        for i, ((h, w), lab) in enumerate(zip(shapes, labels)):
            if seeds is not None:
                seed_both(seeds[i])
            seen.clear()
            ch._draw()
            img, lab = iop.GeoImage.of(h, w), np.asarray(lab)
            for t in (ch.random_horizontal_flip, ch.random_vertical_flip, ch.random_rotate):
                img, lab = t(img, lab)
            rh, rw = img.shape[:2]                              # the rotated image
            img, lab = ch.random_patch(img, lab)
            ph, pw = img.shape[:2]
            # the boxes Resize's filter will see, worked out here: rounded to the output grid
            bx = np.round(lab[:, [lf['xmin'], lf['xmax']]] * (ch.resize.out_width / pw))
            by = np.round(lab[:, [lf['ymin'], lf['ymax']]] * (ch.resize.out_height / ph))
            small = (bx[:, 1] > bx[:, 0]) & (by[:, 1] > by[:, 0]) & ((bx[:, 1] - bx[:, 0]) * (by[:, 1] - by[:, 0]) < 16)
            img, out = ch.resize(img, lab)
            patch = seen.get("patch")
            kind = None
            if patch is not None:
                top, left, p_h, p_w = patch
                in_y, in_x = top >= 0 and top + p_h <= rh, left >= 0 and left + p_w <= rw
                over_y, over_x = top <= 0 and top + p_h >= rh and p_h > rh, left <= 0 and left + p_w >= rw and p_w > rw
                kind = ("inside" if in_y and in_x else "larger" if over_y and over_x else "crop_y_pad_x" if in_y and over_x
                        else "pad_y_crop_x" if over_y and in_x else "other")
            rows.append(dict(hflip=bool(seen.get("horizontal")), vflip=bool(seen.get("vertical")), angle=seen.get("angle", 0),
                             patch=patch, kind=kind, trial=seen.get("trial", 0) if patch is not None else 0,
                             patch_dropped=seen.get("patch_dropped", 0), min_area_dropped=int(small.sum()),
                             resize_dropped=len(lab) - len(out), left=len(out)))
    finally:
        CropPad.__call__, Flip.__call__, Rotate.__call__, ImageValidator.validate_patches = real_cut, real_flip, real_rotate, real_validate
        np.random.set_state(saved)
        random.setstate(saved_py)
    return rows


def branches(rows):
    """The branch table's entries that occur in `rows`."""
    found = set()
    for r in rows:
        found.add("rotation_%d" % r["angle"] if r["angle"] else "rotation_off")
        found.add("hflip_on" if r["hflip"] else "hflip_off")
        found.add("vflip_on" if r["vflip"] else "vflip_off")
        if r["angle"] and r["hflip"]:
            found.add("rotation_with_hflip")
        if r["angle"] and r["vflip"]:
            found.add("rotation_with_vflip")
        if r["angle"] and r["patch"] is not None:
            found.add("rotated_" + r["kind"])
        if r["patch"] is not None:
            found.add("trial_%d" % r["trial"])
        if r["patch_dropped"]:
            found.add("patch_filter_removed_a_box")
        if r["min_area_dropped"] and r["resize_dropped"]:
            found.add("min_area_removed_a_box")
        if r["left"] == 0:
            found.add("no_boxes_left")
    return found


BRANCHES = {"rotation_off", "rotation_90", "rotation_180", "rotation_270", "hflip_on", "hflip_off", "vflip_on", "vflip_off",
            "rotation_with_hflip", "rotation_with_vflip", "rotated_inside", "rotated_larger", "rotated_crop_y_pad_x",
            "rotated_pad_y_crop_x", "trial_1", "trial_2", "trial_3", "patch_filter_removed_a_box", "min_area_removed_a_box",
            "no_boxes_left"}


# ---- the ten golden satellite cases of tests/golden/affine_ops.npz (generated from the reference) ---------------------------------------
def golden_cases():
    """[(case, image, labels, fixture entries)] for seeds 740 .. 749 of tests/affine_cases.py: 40 x 48 images, out 30 x 36."""
    z = util.load("affine_ops")
    out = []
    for i, case in enumerate(ac.CASES):
        if case["op"] != "DataAugmentationSatellite":
            continue
        img, labels = make_inputs(case["seed"], case["n_boxes"], float_labels=case["labels"] == "float", size=(40, 48))
        pre = "a%03d_" % i
        out.append((case, img, labels, {k[len(pre):]: z[k] for k in z.files if k.startswith(pre) and k != pre + "case"}))
    assert [c[0]["seed"] for c in out] == list(range(740, 750))
    return out


np_state_digest = vc.np_state_digest


def py_state_digest():
    return hashlib.sha256(np.asarray(random.getstate()[1], dtype=np.uint32).astype("<u4").tobytes()).hexdigest()


# ---- NumPy stand-ins for the kernels: the host logic without a GPU -----------------------------------------------------------------
def install_cpu_kernels(monkeypatch, calls=None):
    """tests/variable_chain_cases.install_cpu_kernels, plus cv2.warpAffine on NumPy images (tests/np_warp.py), the satellite chain's
    decision exports by tests/np_satellite_chain.py and its plan / gather launches by that module's `geometry`.  calls: a list that
    receives the name of every decision launch."""
    import torch
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.data_generator import _image_ops as iop
    from tests import np_warp
    vc.install_cpu_kernels(monkeypatch)
    real_warp = iop.warp_affine

    def warp_affine(image, M, dsize, background=0):
        if isinstance(image, np.ndarray):
            return np_warp.warp_affine(np.ascontiguousarray(image), M, (int(dsize[0]), int(dsize[1])), background)
        return real_warp(image, M, dsize, background)

    def sat_augment_decide(params, turns, mt_states, labels, n_labels, device, table=None):
        if calls is not None:
            calls.append("decide" if mt_states.ndim == 2 else "stream" if table is None else "stream_ragged")
        B = labels.shape[0]
        shapes = ([(params["img_height"], params["img_width"])] * B if table is None
                  else [(int(r[1]), int(r[2])) for r in np.asarray(table)])
        ops, args, geo, lab_out, n_out, mt_out = nsc.walk(params, np.asarray(turns), mt_states, labels, n_labels, shapes)
        return ops, args, geo, lambda: (geo, lab_out, n_out, mt_out)

    def sat_augment_plans(geo, out_h, out_w, n_taps, size=None, table=None):
        return geo, None, None, None, None, None               # the stand-in gather reads the geometry rows themselves

    def image_resize_gather_turn_u8(images, table, out_h, out_w, plans, ix, wx, iy, wy, transposed, background):
        bg = np.asarray(background)
        return torch.from_numpy(np.stack([nsc.geometry(np.asarray(im), plans[b], out_h, out_w, bg[b]) for b, im in enumerate(images)]))

    def gather_batch_ragged(packed, lazies):
        return torch.from_numpy(np.stack([nsc.execute_lazy(im, lazy) for im, lazy in zip(packed.data, lazies)]))

    monkeypatch.setattr(iop, "warp_affine", warp_affine)
    monkeypatch.setattr(iop, "gather_batch_ragged", gather_batch_ragged)
    monkeypatch.setattr(nat, "sat_augment_decide", sat_augment_decide)
    monkeypatch.setattr(nat, "sat_augment_plans", sat_augment_plans)
    monkeypatch.setattr(nat, "image_resize_gather_turn_u8", image_resize_gather_turn_u8)
