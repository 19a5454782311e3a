"""What the augmentation chains' `augment_batch` routes share (data_augmentation_chain_*.py): the batch argument parser, the label buffers
of the decision kernels, np.random's MT19937 state in the (625,) uint32 layout those kernels step, the cached background rows of the
gathers, the host loop on lazy images and the control flow around the four routes -- seeded / global stream, device / host.

`_native`'s wrappers and `_image_ops`' functions are looked up when they are called (`nat.<name>`, `iop.<name>`), never bound at import:
the CPU suites replace them with NumPy restatements."""
from __future__ import annotations

import ctypes
import os
import random

import numpy as np

from .. import _native as nat
from . import _image_ops as iop
from .object_detection_2d_image_boxes_validation_utils import BoxFilter, ImageValidator
from .object_detection_2d_patch_sampling_ops import PatchCoordinateGenerator


# ---- np.random's generator as the decision kernels take it: 624 key words + the position ---------------------------------------------
def _seed_states(seeds):
    """(B, 625) uint32: per seed the MT19937 state `np.random.seed(seed)` leaves in the global generator (624 key words + the position),
    without touching that generator.  `RandomState.get_state()` builds its tuple in 50 - 180 us, more than the rest of a seeded batch
    takes per image, so the words are read where NumPy keeps them (`MT19937().ctypes.state_address`: uint32 key[624], int pos); the
    first row of every call is held against `get_state()`, and if NumPy ever lays the state out differently all rows come from it."""
    bit_generator = np.random.MT19937()
    rs = np.random.RandomState(bit_generator)
    out = np.empty((len(seeds), 625), dtype=np.uint32)
    direct = True
    for i, seed in enumerate(seeds):
        rs.seed(int(seed))
        if direct:
            out[i] = np.frombuffer(ctypes.string_at(bit_generator.ctypes.state_address, 2500), dtype=np.uint32)
        if i == 0 or not direct:
            st = rs.get_state()
            if i == 0 and not (np.array_equal(out[0, :624], st[1]) and int(out[0, 624]) == st[2]):
                direct = False
            if not direct:
                out[i, :624], out[i, 624] = st[1], st[2]
    return out


def read_np_state():
    """np.random's state as (the bit generator's name, mt (625,) uint32, the rest of `get_state()`'s tuple)."""
    state = np.random.get_state()
    mt = np.empty((625,), dtype=np.uint32)
    mt[:624], mt[624] = state[1], state[2]
    return state[0], mt, state[3:]


def put_np_state(name, mt, rest):
    """np.random goes on from the (625,) state `mt` (`name`, `rest`: read_np_state's)."""
    np.random.set_state((name, mt[:624], int(mt[624])) + tuple(rest))


def record_np_state(states, i):
    """states[i] = where np.random stands now (the state behind image i of a seeded batch)."""
    st = np.random.get_state()
    states[i, :624], states[i, 624] = st[1], st[2]


# ---- labels: a list of (n_i, 5) arrays <-> the kernels' (B, AUG_MAX_BOXES, 5) float64 buffer in class, xmin, ymin, xmax, ymax order ---
def label_cols(labels_format):
    return [labels_format[k] for k in ('class_id', 'xmin', 'ymin', 'xmax', 'ymax')]


def labels_fit(labels):
    """The layout the decision kernels take: arrays of ONE dtype, int64 or float64, each (n, 5) with at most `nat.AUG_MAX_BOXES` rows."""
    arrs = [np.asarray(lab) for lab in labels]
    dtypes = {a.dtype for a in arrs}
    return (len(dtypes) == 1 and next(iter(dtypes)) in (np.dtype(np.int64), np.dtype(np.float64))
            and all(a.ndim == 2 and a.shape[1] == 5 and a.shape[0] <= nat.AUG_MAX_BOXES for a in arrs))


def _filled(n):
    """(B, AUG_MAX_BOXES) bool: the first n[i] rows of image i."""
    return np.arange(nat.AUG_MAX_BOXES)[None, :] < np.asarray(n)[:, None]


def pack_labels(labels, cols):
    """-> (the labels as arrays, lab_in (B, AUG_MAX_BOXES, 5) float64 with the columns in `cols` order, n_in (B,) int32)."""
    arrs = [np.asarray(lab) for lab in labels]
    lab_in = np.zeros((len(arrs), nat.AUG_MAX_BOXES, 5), dtype=np.float64)
    n_in = np.array([a.shape[0] for a in arrs], dtype=np.int32)
    if n_in.any():
        lab_in[_filled(n_in)] = np.concatenate(arrs)[:, cols]            # image after image, row after row: the mask's own order
    return arrs, lab_in, n_in


def unpack_labels(lab_out, n_out, cols, dtype):
    """pack_labels' inverse on the kernels' output: a list of (n_out[i], 5) arrays, columns back where `cols` took them from."""
    rows = lab_out[_filled(n_out)][:, np.argsort(cols)].astype(dtype, order='C')
    return np.split(rows, np.cumsum(n_out)[:-1])


# ---- augment_batch's arguments ------------------------------------------------------------------------------------------------------
def is_cuda_batch(images):
    import torch
    return torch.is_tensor(images) and images.is_cuda and images.dtype == torch.uint8 and images.dim() == 4 and images.shape[3] == 3


def parse_batch(images, labels, seeds=None, lists=True):
    """images: a list of (H_i, W_i, 3) uint8 images (`lists`: the chain takes them; one ragged upload, `iop.pack_ragged`) or a
    (B, H, W, 3) CUDA uint8 batch; one label array and, with `seeds`, one seed per image.  -> (batch | None, packed | None, [(H, W)])."""
    if lists and isinstance(images, (list, tuple)):
        if any(len(im.shape) != 3 or int(im.shape[2]) != 3 for im in images):
            raise TypeError("augment_batch takes a list of (H, W, 3) uint8 images")
        if len(labels) != len(images):
            raise ValueError("one label array per image")
        batch, packed = None, iop.pack_ragged(list(images))
        shapes = [(h, w) for h, w, _ in packed.shapes]
    else:
        if not is_cuda_batch(images):
            raise TypeError("augment_batch takes a list of (H, W, 3) uint8 images or a (B, H, W, 3) CUDA uint8 batch" if lists
                            else "augment_batch takes a (B, H, W, 3) CUDA uint8 batch")
        if len(labels) != images.shape[0]:
            raise ValueError("one label array per image")
        batch, packed = images, None
        shapes = [(int(images.shape[1]), int(images.shape[2]))] * int(images.shape[0])
    if seeds is not None and len(seeds) != len(shapes):
        raise ValueError("one seed per image")
    return batch, packed, shapes


def background_rows(chain, B, device, colour):
    """(B, 3) uint8 CUDA tensor of `colour`, what the gathers and the warp take as their background: uploaded once per (B, device,
    colour) and kept in chain.__dict__["_bg_rows"]."""
    key = (B, str(device), tuple(int(v) for v in colour))
    bg = chain.__dict__.get("_bg_rows")
    if bg is None or bg[0] != key:
        bg = (key, nat.to_device(np.repeat(np.array(key[2], dtype=np.uint8)[None], B, 0), device=device))
        chain.__dict__["_bg_rows"] = bg
    return bg[1]


# ---- the host route: the ops' own code on lazy images, the pixels of the batch in two launches --------------------------------------
def host_batch(batch, packed, shapes, labels, seeds, draw, lazy, reseed=np.random.seed):
    """Per image: `draw()` -> (its pixel program, its geometric transforms), the transforms on the lazy image `lazy.of(h, w)` (`lazy`:
    iop.GeoImage or iop.WarpImage) that only records them -- under `reseed(seeds[i])` when `seeds` is given -- then the programs and
    the recorded geometry of the whole batch in two launches, on the CUDA batch `batch` or the ragged batch `packed`.  Returns (batch,
    labels, the np.random state behind each image (B, 625) | None without seeds)."""
    programs, lazies, out_labels = [], [], []
    states = None if seeds is None else np.empty((len(shapes), 625), dtype=np.uint32)
    for i, ((h, w), lab) in enumerate(zip(shapes, labels)):
        if seeds is not None:
            reseed(int(seeds[i]))
        program, transforms = draw()
        img = lazy.of(h, w)
        for transform in transforms:
            img, lab = transform(img, lab)
        programs.append(program)
        lazies.append(img)
        out_labels.append(lab)
        if seeds is not None:
            record_np_state(states, i)
    if packed is not None:
        return iop.gather_batch_ragged(iop.run_ragged(packed, programs), lazies), out_labels, states
    finish = iop.warp_batch if lazy is iop.WarpImage else iop.gather_batch
    return finish(iop.run_batch(batch, programs), lazies), out_labels, states


def reseed_both(seed):
    """A seeded image of a chain that also draws from Python's `random` (RandomRotate's angle)."""
    np.random.seed(seed)
    random.seed(seed)


# ---- the control flow of augment_batch ----------------------------------------------------------------------------------------------
def augment_batch(chain, images, labels, seeds, lists=True, ahead=None, behind=None, loop=None, python_random=False):
    """`chain.augment_batch`, for a chain with `_sync_formats`, `_device_params(labels, generator=, shapes=)`, `_augment_batch_device(batch,
    packed, shapes, labels, params, mt, *drawn ahead) -> (batch, labels, state(s), *more)` and `_augment_batch_host(batch, packed, shapes,
    labels, seeds) -> (batch, labels, states)`:

    seeds given: the device route on `_seed_states(seeds)` where `_device_params` covers the batch, else the host route under each seed
    with the global generator(s) saved and put back; either way `_last_generator_states` is the state behind each image.
    seeds None: the device route on np.random's own state, put back afterwards, unless SSDHIP_AUG_HOST_STREAM=1 or `_device_params`
    says no; else the host route on the global stream.

    The hooks: `ahead(seeds | None, B)` -> what is drawn on the host in front of the device route and handed to it behind `mt`;
    `behind(*more)` runs after a global-stream device batch (the other generator catches up); `loop(images, labels, seeds)` takes over,
    from the generator state(s) the host route started on, when that raises NotImplementedError; `python_random`: Python's `random` is
    saved and restored beside np.random."""
    batch, packed, shapes = parse_batch(images, labels, seeds, lists)
    B = len(shapes)
    chain._sync_formats()

    def save():
        return np.random.get_state(), random.getstate() if python_random else None

    def restore(saved):
        np.random.set_state(saved[0])
        if python_random:
            random.setstate(saved[1])

    def host(seeds):
        if loop is None:
            return chain._augment_batch_host(batch, packed, shapes, labels, seeds)
        saved = save()
        try:
            return chain._augment_batch_host(batch, packed, shapes, labels, seeds)
        except NotImplementedError:
            restore(saved)
            return loop(images, labels, seeds)

    if seeds is not None:
        params = chain._device_params(labels, shapes=shapes) if B else None
        if params is not None:
            drawn = () if ahead is None else ahead(seeds, B)
            out, out_labels, mt_out = chain._augment_batch_device(batch, packed, shapes, labels, params, _seed_states(seeds), *drawn)[:3]
        else:
            saved = save()
            try:
                out, out_labels, mt_out = host(seeds)
            finally:
                restore(saved)
        chain.__dict__["_last_generator_states"] = mt_out
        return out, out_labels
    if os.environ.get("SSDHIP_AUG_HOST_STREAM", "0") != "1" and B:
        name, mt, rest = read_np_state()
        params = chain._device_params(labels, generator=name, shapes=shapes)
        if params is not None:
            drawn = () if ahead is None else ahead(None, B)
            out, out_labels, mt_out, *more = chain._augment_batch_device(batch, packed, shapes, labels, params, mt, *drawn)
            put_np_state(name, mt_out, rest)                             # the stream goes on behind the batch
            if behind is not None:
                behind(*more)
            return out, out_labels
    return host(None)[:2]


# ---- the variable-input-size and satellite chains: photometric program -> [flips, turn] -> RandomPatch -> Resize ------------------------
def is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def is_whole(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, bool)


def photo_program(chain):
    """One image's photometric draws in the order of the two chains' `transformations` -> its pixel program."""
    return ([("to_f32", 0)] + chain.random_brightness.draw() + chain.random_contrast.draw() + [("to_u8", 0), ("rgb2hsv", 0), ("to_f32", 0)]
            + chain.random_saturation.draw() + chain.random_hue.draw() + [("to_u8", 0), ("hsv2rgb", 0)])


def patch_n_taps(chain, shapes, turned=False):
    """Taps per output pixel the device-built tables need for images of these (H, W): eight (Lanczos-4's) unless Resize runs in
    INTER_AREA, whose true area filter takes ceil(source / output extent) + 2 of the largest possible patch.  `turned`: a rotation may
    swap height and width, so both are taken as the largest side of any image."""
    if int(chain.resize.interpolation_mode) != iop.INTER_AREA:
        return 8
    gen = chain.random_patch.patch_coord_generator
    h_max, w_max = max(s[0] for s in shapes), max(s[1] for s in shapes)
    if turned:
        h_max = w_max = max(h_max, w_max)
    pw = float(gen.max_scale) * w_max
    ph = pw / float(gen.min_aspect_ratio)
    return max(8, int(np.ceil(max(max(ph, h_max) / chain.resize.out_height, max(pw, w_max) / chain.resize.out_width))) + 2)


def patch_device_params(chain, flips, labels, generator, shapes, turned=False):
    """The fields of ssdhip_var_augment_params (without the image size) of a chain whose geometry is `flips` ((RandomFlip, its dim), ...;
    `flip_prob` is the first one's), `chain.random_patch` and `chain.resize`, or None for anything the decision kernels
    (csrc/ssdhip_augment.hip) do not cover; DataAugmentationVariableInputSize._device_params lists what that is.  `turned`: the size
    conditions are taken over the smaller side of every image, because a rotation swaps height and width."""
    rp, rs = chain.random_patch, chain.resize
    gen, sp, val, bfr = rp.patch_coord_generator, rp.sample_patch, rp.image_validator, rs.box_filter
    bf = sp.box_filter
    photo = (chain.random_brightness, chain.random_contrast, chain.random_saturation, chain.random_hue)
    number, whole = is_number, is_whole
    pair = lambda v: isinstance(v, (list, tuple)) and len(v) == 2 and number(v[0]) and number(v[1]) and v[0] <= v[1]
    ok = (generator == 'MT19937'
          and isinstance(bf, BoxFilter) and isinstance(val, ImageValidator) and isinstance(bfr, BoxFilter)
          and isinstance(gen, PatchCoordinateGenerator)
          and bf.overlap_criterion == val.overlap_criterion and bf.overlap_criterion in nat.VAR_AUG_CRITERION
          and bf.border_pixels == 'half' and val.border_pixels == 'half'
          and bf.check_overlap and not bf.check_min_area and not bf.check_degenerate
          and not bfr.check_overlap and bfr.check_min_area and bfr.check_degenerate and number(bfr.min_area)
          and pair(bf.overlap_bounds) and pair(val.bounds)
          and (val.n_boxes_min == 'all' or (whole(val.n_boxes_min) and val.n_boxes_min >= 1))
          and whole(rp.n_trials_max) and rp.n_trials_max >= 0 and not rp.can_fail
          and gen.must_match == 'w_ar' and not gen.scale_uniformly
          and all(v is None for v in (gen.patch_ymin, gen.patch_xmin, gen.patch_height, gen.patch_width, gen.patch_aspect_ratio))
          and number(gen.min_scale) and number(gen.max_scale) and 0 < gen.min_scale < gen.max_scale
          and number(gen.min_aspect_ratio) and number(gen.max_aspect_ratio) and 0 < gen.min_aspect_ratio < gen.max_aspect_ratio
          and all(number(op.prob) and 0.0 <= op.prob <= 1.0 for op in photo + (rp,) + tuple(fl for fl, _ in flips))
          and all(fl.dim == dim for fl, dim in flips)
          and whole(rs.interpolation_mode) and 0 <= rs.interpolation_mode <= 4
          and whole(rs.out_height) and whole(rs.out_width) and rs.out_height > 0 and rs.out_width > 0
          and sorted(chain.labels_format.get(k, -1) for k in ('class_id', 'xmin', 'ymin', 'xmax', 'ymax')) == [0, 1, 2, 3, 4])
    if ok:
        try:
            ok = len(tuple(int(v) for v in sp.background)) == 3
        except (TypeError, ValueError):
            ok = False
    if ok and labels is not None:
        ok = labels_fit(labels)
    if ok and shapes is not None:
        h_min, w_min = min(s[0] for s in shapes), min(s[1] for s in shapes)
        if turned:
            h_min = w_min = min(h_min, w_min)
        # the narrowest patch is int(min_scale * W) wide and int(width / aspect ratio) high: both must stay >= 1, whichever side is W
        ok = (w_min >= 4 and h_min >= 1 and int(gen.min_scale * w_min) >= max(1.0, gen.max_aspect_ratio) and chain._n_taps(shapes) <= 64)
    if not ok:
        return None
    return dict(photo_prob=[float(op.prob) for op in photo],
                photo_lower=[float(op.lower) for op in photo[:3]] + [-float(chain.random_hue.max_delta)],
                photo_upper=[float(op.upper) for op in photo[:3]] + [float(chain.random_hue.max_delta)],
                patch_prob=float(rp.prob), min_scale=float(gen.min_scale), max_scale=float(gen.max_scale),
                min_aspect_ratio=float(gen.min_aspect_ratio), max_aspect_ratio=float(gen.max_aspect_ratio),
                n_trials=int(rp.n_trials_max), clip_boxes=int(bool(sp.clip_boxes)),
                criterion=int(nat.VAR_AUG_CRITERION[bf.overlap_criterion]),
                n_boxes_min=0 if val.n_boxes_min == 'all' else int(val.n_boxes_min),
                validator_lower=float(val.bounds[0]), validator_upper=float(val.bounds[1]),
                filter_lower=float(bf.overlap_bounds[0]), filter_upper=float(bf.overlap_bounds[1]), flip_prob=float(flips[0][0].prob),
                out_height=int(rs.out_height), out_width=int(rs.out_width), interpolation=int(rs.interpolation_mode),
                resize_min_area=float(bfr.min_area))


def patch_device_batch(chain, batch, packed, shapes, labels, params, mt, turns=None):
    """The four launches behind the two chains' `_device_params`: decisions (mt (B, 625) = one generator state per image, (625,) = one
    for the batch; turns (B,) | None: the satellite chain's quarter turns, which select its exports), the photometric programs read from
    the device, the tap tables and the gather -- on the CUDA batch `batch`, or on the ragged batch `packed`; ONE download at the end.
    Returns (batch, labels, generator state(s), the geometry rows)."""
    import torch
    B = len(shapes)
    cols = label_cols(chain.labels_format)
    arrs, lab_in, n_in = pack_labels(labels, cols)
    out_h, out_w, n_taps = int(chain.resize.out_height), int(chain.resize.out_width), chain._n_taps(shapes)
    device = batch.device if packed is None else packed.data.device
    bg = background_rows(chain, B, device, chain.random_patch.sample_patch.background)
    table = None if packed is None else packed.table
    if packed is None:
        params = dict(params, img_height=shapes[0][0], img_width=shapes[0][1])
    if turns is None:
        ops_dev, args_dev, geo_dev, fetch = nat.var_augment_decide(params, mt, lab_in, n_in, device, table=table)
    else:
        ops_dev, args_dev, geo_dev, fetch = nat.sat_augment_decide(params, turns, mt, lab_in, n_in, device, table=table)
    if packed is None:
        distorted = nat.image_program(batch.contiguous(), ops_dev, args_dev, torch.uint8)
    else:
        distorted = nat.image_program_ragged_u8(packed.data, table, packed.max_pixels, ops_dev, args_dev)
    if turns is not None:
        plans, ix, wx, iy, wy, tr = nat.sat_augment_plans(geo_dev, out_h, out_w, n_taps, size=shapes[0] if packed is None else None,
                                                          table=table)
        out = nat.image_resize_gather_turn_u8(distorted, table, out_h, out_w, plans, ix, wx, iy, wy, tr, bg)
    elif packed is None:
        plans, ix, wx, iy, wy = nat.augment_plans(geo_dev, shapes[0][0], shapes[0][1], out_h, out_w, n_taps)
        out = nat.image_resize_gather_cv_u8(distorted, out_h, out_w, plans, ix, wx, iy, wy, bg)
    else:
        plans, ix, wx, iy, wy = nat.augment_plans_ragged(geo_dev, table, out_h, out_w, n_taps)
        out = nat.image_resize_gather_ragged_u8(distorted, table, out_h, out_w, plans, ix, wx, iy, wy, bg)
    geo, lab_out, n_out, mt_out = fetch()
    return out, unpack_labels(lab_out, n_out, cols, arrs[0].dtype), mt_out, geo
