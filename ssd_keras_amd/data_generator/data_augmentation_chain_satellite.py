"""Drop-in for the reference's data_generator/data_augmentation_chain_satellite.py: `DataAugmentationSatellite`, a chain for images in
bird's eye view -- photometric distortions, random horizontal and vertical flips, a random rotation by 90 / 180 / 270 degrees
(`RandomRotate`, cv2.warpAffine), a random patch and the resize to the network input -- built from the package's ops.

`__call__` runs the reference's list of transforms on one image, its pixels on the GPU one op at a time.  `augment_batch` does the same
for a batch -- a list of images of any sizes (one ragged upload) or a CUDA batch of one size -- in THREE pixel launches, as the
variable-input-size chain does: every image's photometric program, the tap tables of resize <- patch <- rotation <- flips built on the
device, and one gather.  A rotation by quarter turns under the reference's matrix is an exact index permutation with a border of zeros,
so a rotated image is still two index maps, with one "transposed" bit for 90 / 270 degrees.  The draws, the validation of every patch
trial and the label arithmetic run on the device (csrc/ssdhip_augment.hip: `ssdhip_sat_augment_decide[_stream[_ragged]]` on NumPy's
MT19937 stream); `RandomRotate`'s angle, the chain's one draw from Python's `random`, is drawn B times in advance on the host from a copy
of that generator, and the real generator then advances by as many `random.choice` calls as images rotated.  What the kernel does not
cover (`_device_params`) runs the ops' own host code on lazy images (`_image_ops.GeoImage`), and what that cannot express either runs
the `__call__` loop.  Every route gives the `__call__` loop's results, bit for bit.

As in the reference, `__call__` without labels reaches for a `sequence1` the class never defines and raises AttributeError (:155), and the
`background` argument never reaches RandomPatch: what a patch adds around an image is RandomPatch's own default, black."""
from __future__ import annotations

import random

import numpy as np

from . import _image_ops as iop
from .data_augmentation_chain_constant_input_size import _seed_states
from .object_detection_2d_geometric_ops import RandomFlip, RandomRotate, Resize
from .object_detection_2d_image_boxes_validation_utils import BoxFilter, ImageValidator
from .object_detection_2d_patch_sampling_ops import PatchCoordinateGenerator, RandomPatch
from .object_detection_2d_photometric_ops import (ConvertColor, ConvertDataType, ConvertTo3Channels, RandomBrightness, RandomContrast,
                                                  RandomHue, RandomSaturation)


class DataAugmentationSatellite:
    '''Photometric and geometric transformations for images without an "up" or "down" (reference :28-157).'''

    def __init__(self,
                 resize_height,
                 resize_width,
                 random_brightness=(-48, 48, 0.5),
                 random_contrast=(0.5, 1.8, 0.5),
                 random_saturation=(0.5, 1.8, 0.5),
                 random_hue=(18, 0.5),
                 random_flip=0.5,
                 random_rotate=([90, 180, 270], 0.5),
                 min_scale=0.3,
                 max_scale=2.0,
                 min_aspect_ratio=0.8,
                 max_aspect_ratio=1.25,
                 n_trials_max=3,
                 clip_boxes=True,
                 overlap_criterion='area',
                 bounds_box_filter=(0.3, 1.0),
                 bounds_validator=(0.5, 1.0),
                 n_boxes_min=1,
                 background=(0, 0, 0),
                 labels_format={'class_id': 0, 'xmin': 1, 'ymin': 2, 'xmax': 3, 'ymax': 4}):
        self.n_trials_max = n_trials_max
        self.clip_boxes = clip_boxes
        self.overlap_criterion = overlap_criterion
        self.bounds_box_filter = bounds_box_filter
        self.bounds_validator = bounds_validator
        self.n_boxes_min = n_boxes_min
        self.background = background
        self.labels_format = labels_format

        self.box_filter_patch = BoxFilter(check_overlap=True, check_min_area=False, check_degenerate=False,
                                          overlap_criterion=self.overlap_criterion, overlap_bounds=self.bounds_box_filter,
                                          labels_format=self.labels_format)
        self.box_filter_resize = BoxFilter(check_overlap=False, check_min_area=True, check_degenerate=True, min_area=16,
                                           labels_format=self.labels_format)
        self.image_validator = ImageValidator(overlap_criterion=self.overlap_criterion, bounds=self.bounds_validator,
                                              n_boxes_min=self.n_boxes_min, labels_format=self.labels_format)

        self.convert_to_3_channels = ConvertTo3Channels()
        self.convert_RGB_to_HSV = ConvertColor(current='RGB', to='HSV')
        self.convert_HSV_to_RGB = ConvertColor(current='HSV', to='RGB')
        self.convert_to_float32 = ConvertDataType(to='float32')
        self.convert_to_uint8 = ConvertDataType(to='uint8')
        self.resize = Resize(height=resize_height, width=resize_width, box_filter=self.box_filter_resize, labels_format=self.labels_format)

        self.random_brightness = RandomBrightness(lower=random_brightness[0], upper=random_brightness[1], prob=random_brightness[2])
        self.random_contrast = RandomContrast(lower=random_contrast[0], upper=random_contrast[1], prob=random_contrast[2])
        self.random_saturation = RandomSaturation(lower=random_saturation[0], upper=random_saturation[1], prob=random_saturation[2])
        self.random_hue = RandomHue(max_delta=random_hue[0], prob=random_hue[1])

        self.random_horizontal_flip = RandomFlip(dim='horizontal', prob=random_flip, labels_format=self.labels_format)
        self.random_vertical_flip = RandomFlip(dim='vertical', prob=random_flip, labels_format=self.labels_format)
        self.random_rotate = RandomRotate(angles=random_rotate[0], prob=random_rotate[1], labels_format=self.labels_format)
        self.patch_coord_generator = PatchCoordinateGenerator(must_match='w_ar', min_scale=min_scale, max_scale=max_scale, scale_uniformly=False,
                                                              min_aspect_ratio=min_aspect_ratio, max_aspect_ratio=max_aspect_ratio)
        self.random_patch = RandomPatch(patch_coord_generator=self.patch_coord_generator, box_filter=self.box_filter_patch,
                                        image_validator=self.image_validator, n_trials_max=self.n_trials_max, clip_boxes=self.clip_boxes,
                                        prob=1.0, can_fail=False, labels_format=self.labels_format)

        self.transformations = [self.convert_to_3_channels, self.convert_to_float32, self.random_brightness, self.random_contrast,
                                self.convert_to_uint8, self.convert_RGB_to_HSV, self.convert_to_float32, self.random_saturation,
                                self.random_hue, self.convert_to_uint8, self.convert_HSV_to_RGB, self.random_horizontal_flip,
                                self.random_vertical_flip, self.random_rotate, self.random_patch, self.resize]

    def _sync_formats(self):
        self.random_patch.labels_format = self.labels_format
        self.random_horizontal_flip.labels_format = self.labels_format
        self.random_vertical_flip.labels_format = self.labels_format
        self.random_rotate.labels_format = self.labels_format
        self.resize.labels_format = self.labels_format

    def __call__(self, image, labels=None):
        self._sync_formats()
        if labels is not None:
            for transform in self.transformations:
                image, labels = transform(image, labels)
            return image, labels
        for transform in self.sequence1:
            image = transform(image)
        return image

    def _draw(self):
        """One image's photometric draws in the order of `transformations` -> its pixel program."""
        return ([("to_f32", 0)] + self.random_brightness.draw() + self.random_contrast.draw() + [("to_u8", 0), ("rgb2hsv", 0), ("to_f32", 0)]
                + self.random_saturation.draw() + self.random_hue.draw() + [("to_u8", 0), ("hsv2rgb", 0)])

    def _n_taps(self, shapes):
        """Taps per output pixel the device-built tables need for images of these (H, W): eight (Lanczos-4's) unless Resize runs in
        INTER_AREA, whose true area filter takes ceil(source / output extent) + 2 of the largest possible patch -- a rotation may swap
        height and width, so both are taken as the largest side of any image."""
        if int(self.resize.interpolation_mode) != iop.INTER_AREA:
            return 8
        gen = self.random_patch.patch_coord_generator
        side = max(max(s[0], s[1]) for s in shapes)
        pw = float(gen.max_scale) * side
        ph = pw / float(gen.min_aspect_ratio)
        return max(8, int(np.ceil(max(max(ph, side) / self.resize.out_height, max(pw, side) / self.resize.out_width))) + 2)

    def _device_params(self, labels=None, generator='MT19937', shapes=None):
        """The chain's configuration as the fields of ssdhip_sat_augment_params (without the image size), or None for anything the
        decision kernel (csrc/ssdhip_augment.hip) does not cover: what DataAugmentationVariableInputSize._device_params lists, except
        that both flips are allowed, each with its own `dim` and probability in [0, 1] -- and `angles` that are not a non-empty list
        within {90, 180, 270}, a rotation probability outside [0, 1], label arrays that are not int64 or float64 WITH WHOLE-NUMBER
        VALUES (the closed form of Rotate's label arithmetic holds for those only); the size conditions are taken over the smaller and
        the larger side of every image, because a rotation swaps height and width."""
        from .. import _native as nat
        rp, rs, rr = self.random_patch, self.resize, self.random_rotate
        hf, vf = self.random_horizontal_flip, self.random_vertical_flip
        gen, sp, val, bfr = rp.patch_coord_generator, rp.sample_patch, rp.image_validator, rs.box_filter
        bf = sp.box_filter
        photo = (self.random_brightness, self.random_contrast, self.random_saturation, self.random_hue)
        number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)
        whole = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
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
              and all(number(op.prob) and 0.0 <= op.prob <= 1.0 for op in photo + (rp, hf, vf, rr))
              and hf.dim == 'horizontal' and vf.dim == 'vertical'
              and isinstance(rr.angles, (list, tuple)) and len(rr.angles) > 0
              and all(whole(a) and a in (90, 180, 270) for a in rr.angles)
              and whole(rs.interpolation_mode) and 0 <= rs.interpolation_mode <= 4
              and whole(rs.out_height) and whole(rs.out_width) and rs.out_height > 0 and rs.out_width > 0
              and sorted(self.labels_format.get(k, -1) for k in ('class_id', 'xmin', 'ymin', 'xmax', 'ymax')) == [0, 1, 2, 3, 4])
        if ok:
            try:
                ok = len(tuple(int(v) for v in sp.background)) == 3
            except (TypeError, ValueError):
                ok = False
        if ok and labels is not None:
            arrs = [np.asarray(lab) for lab in labels]
            dtypes = {a.dtype for a in arrs}
            ok = (len(dtypes) == 1 and next(iter(dtypes)) in (np.dtype(np.int64), np.dtype(np.float64))
                  and all(a.ndim == 2 and a.shape[1] == 5 and a.shape[0] <= nat.AUG_MAX_BOXES for a in arrs))
            if ok and arrs[0].dtype == np.float64:
                ok = all(bool(np.all(np.isfinite(a)) and np.all(a == np.floor(a)) and np.all(np.abs(a) < 2.0 ** 52)) for a in arrs)
        if ok and shapes is not None:
            side_min = min(min(s[0], s[1]) for s in shapes)
            # the narrowest patch is int(min_scale * W) wide and int(width / aspect ratio) high: both must stay >= 1, whichever side is W
            ok = (side_min >= 4 and int(gen.min_scale * side_min) >= max(1.0, gen.max_aspect_ratio) and self._n_taps(shapes) <= 64)
        if not ok:
            return None
        return dict(photo_prob=[float(op.prob) for op in photo],
                    photo_lower=[float(op.lower) for op in photo[:3]] + [-float(self.random_hue.max_delta)],
                    photo_upper=[float(op.upper) for op in photo[:3]] + [float(self.random_hue.max_delta)],
                    patch_prob=float(rp.prob), min_scale=float(gen.min_scale), max_scale=float(gen.max_scale),
                    min_aspect_ratio=float(gen.min_aspect_ratio), max_aspect_ratio=float(gen.max_aspect_ratio),
                    n_trials=int(rp.n_trials_max), clip_boxes=int(bool(sp.clip_boxes)),
                    criterion=int(nat.VAR_AUG_CRITERION[bf.overlap_criterion]),
                    n_boxes_min=0 if val.n_boxes_min == 'all' else int(val.n_boxes_min),
                    validator_lower=float(val.bounds[0]), validator_upper=float(val.bounds[1]),
                    filter_lower=float(bf.overlap_bounds[0]), filter_upper=float(bf.overlap_bounds[1]), flip_prob=float(hf.prob),
                    out_height=int(rs.out_height), out_width=int(rs.out_width), interpolation=int(rs.interpolation_mode),
                    resize_min_area=float(bfr.min_area), vflip_prob=float(vf.prob), rotate_prob=float(rr.prob))

    def _lazy_of(self, g, h, w):
        """The GeoImage of one image's recorded geometry (a row of ssdhip_sat_augment_decide*'s `geometry`) over an h x w image."""
        img = iop.GeoImage.of(h, w)
        if g[5]:
            img = img[:, ::-1]
        if g[6]:
            img = img[::-1]
        if g[7]:
            img = img.turn(90 * int(g[7]))
        if g[0]:
            img = img.window(int(g[1]), int(g[2]), int(g[3]), int(g[4]), self.random_patch.sample_patch.background)
        return img.resize(self.resize.out_height, self.resize.out_width, int(g[11]))

    def _augment_batch_device(self, batch, packed, shapes, labels, params, mt, turns):
        """The four launches behind `_device_params`: decisions (mt (B, 625) = one generator state per image, (625,) = one for the
        batch; turns (B,): the quarter turns drawn from Python's `random`), the photometric programs read from the device, the tap
        tables and the gather -- on the CUDA batch `batch`, or on the ragged batch `packed`; ONE download at the end.  Returns (batch,
        labels, generator state(s), how many images rotated)."""
        import torch
        from .. import _native as nat
        B = len(shapes)
        lf = self.labels_format
        cols = [lf['class_id'], lf['xmin'], lf['ymin'], lf['xmax'], lf['ymax']]
        arrs = [np.asarray(lab) for lab in labels]
        lab_in = np.zeros((B, nat.AUG_MAX_BOXES, 5), dtype=np.float64)
        n_in = np.empty((B,), dtype=np.int32)
        for i, a in enumerate(arrs):
            n_in[i] = a.shape[0]
            if a.shape[0]:
                lab_in[i, :a.shape[0]] = a[:, cols]
        out_h, out_w, n_taps = int(self.resize.out_height), int(self.resize.out_width), self._n_taps(shapes)
        device = batch.device if packed is None else packed.data.device
        row = tuple(int(v) for v in self.random_patch.sample_patch.background)
        bg = self.__dict__.get("_bg_rows")
        if bg is None or bg[0] != (B, str(device), row):
            bg = ((B, str(device), row), nat.to_device(np.repeat(np.array(row, dtype=np.uint8)[None], B, 0), device=device))
            self.__dict__["_bg_rows"] = bg
        if packed is None:
            h, w = shapes[0]
            ops_dev, args_dev, geo_dev, fetch = nat.sat_augment_decide(dict(params, img_height=h, img_width=w), turns, mt, lab_in, n_in,
                                                                       device)
            distorted = nat.image_program(batch.contiguous(), ops_dev, args_dev, torch.uint8)
            plans, ix, wx, iy, wy, tr = nat.sat_augment_plans(geo_dev, out_h, out_w, n_taps, size=(h, w))
            out = nat.image_resize_gather_turn_u8(distorted, None, out_h, out_w, plans, ix, wx, iy, wy, tr, bg[1])
        else:
            ops_dev, args_dev, geo_dev, fetch = nat.sat_augment_decide(params, turns, mt, lab_in, n_in, device, table=packed.table)
            distorted = nat.image_program_ragged_u8(packed.data, packed.table, packed.max_pixels, ops_dev, args_dev)
            plans, ix, wx, iy, wy, tr = nat.sat_augment_plans(geo_dev, out_h, out_w, n_taps, table=packed.table)
            out = nat.image_resize_gather_turn_u8(distorted, packed.table, out_h, out_w, plans, ix, wx, iy, wy, tr, bg[1])
        geo, lab_out, n_out, mt_out = fetch()
        inv, dt = np.argsort(cols), arrs[0].dtype
        return (out, [np.ascontiguousarray(lab_out[i, :int(n_out[i])][:, inv]).astype(dt) for i in range(B)], mt_out,
                int(np.count_nonzero(np.asarray(geo)[:, 7])))

    def _augment_batch_host(self, batch, packed, shapes, labels, seeds):
        """What `_device_params` does not cover: per image the photometric draws, then the two flips, RandomRotate, RandomPatch and
        Resize's own code on a lazy image -- under the image's seed (both generators) when `seeds` is given -- and the pixels of the
        batch in two launches.  Raises NotImplementedError for a geometry lazy images cannot record.  Returns (batch, labels, the
        np.random state behind each image (B, 625) | None without seeds)."""
        programs, lazies, out_labels = [], [], []
        states = None if seeds is None else np.empty((len(shapes), 625), dtype=np.uint32)
        for i, ((h, w), lab) in enumerate(zip(shapes, labels)):
            if seeds is not None:
                np.random.seed(int(seeds[i]))
                random.seed(int(seeds[i]))
            programs.append(self._draw())
            img = iop.GeoImage.of(h, w)
            for transform in (self.random_horizontal_flip, self.random_vertical_flip, self.random_rotate, self.random_patch, self.resize):
                img, lab = transform(img, lab)
            lazies.append(img)
            out_labels.append(lab)
            if seeds is not None:
                st = np.random.get_state()
                states[i, :624], states[i, 624] = st[1], st[2]
        if packed is None:
            return iop.gather_batch(iop.run_batch(batch, programs), lazies), out_labels, states
        return iop.gather_batch_ragged(iop.run_ragged(packed, programs), lazies), out_labels, states

    def _augment_batch_loop(self, images, labels, seeds):
        """The `__call__` loop itself, for what neither batch route can express: (batch, labels, states | None)."""
        import torch
        from .. import _native as nat
        out, out_labels = [], []
        states = None if seeds is None else np.empty((len(labels), 625), dtype=np.uint32)
        for i, lab in enumerate(labels):
            img = images[i]
            img = img if isinstance(img, np.ndarray) else img.cpu().numpy()
            if seeds is not None:
                np.random.seed(int(seeds[i]))
                random.seed(int(seeds[i]))
            px, lb = self(img, lab)
            out.append(px)
            out_labels.append(lb)
            if seeds is not None:
                st = np.random.get_state()
                states[i, :624], states[i, 624] = st[1], st[2]
        device = images.device if torch.is_tensor(images) else None
        return nat.to_device(np.stack(out), device=device), out_labels, states

    def augment_batch(self, images, labels, seeds=None):
        """The chain on a batch: images a list of (H_i, W_i, 3) uint8 NumPy arrays / CUDA tensors of any sizes (they cross PCIe in one
        copy) or a (B, H, W, 3) CUDA uint8 batch, labels a list of B (n_i, 5) arrays -> ((B, resize_height, resize_width, 3) CUDA uint8
        batch, list of B label arrays in the labels' dtype and column order).

        `seeds=None`: every random draw is the one a loop of `__call__` over the batch makes on the global generators, and np.random and
        Python's `random` both end where that loop leaves them.  The draws, the validation of every patch trial and the label arithmetic
        run on the device (`ssdhip_sat_augment_decide_stream[_ragged]`: one wave walks the batch on np.random's MT19937 state, which is
        put back afterwards; the angles come from a copy of `random`'s generator, which then makes as many `random.choice(angles)` calls
        as images rotated); `SSDHIP_AUG_HOST_STREAM=1`, or anything `_device_params` does not cover, takes the ops' host code instead
        -- same results.

        `seeds=[s_0, ...]`: image i comes out exactly as `np.random.seed(s_i); random.seed(s_i); chain(image_i, labels_i)` gives it,
        every image on its own stream (`ssdhip_sat_augment_decide`: one wave per image), both global generators untouched, lists of
        mixed sizes included; `_last_generator_states` (B, 625) holds np.random's state behind each image.  What `_device_params` does
        not cover runs the host code under each seed."""
        import os
        import torch
        if isinstance(images, (list, tuple)):
            if any(len(im.shape) != 3 or int(im.shape[2]) != 3 for im in images):
                raise TypeError("augment_batch takes a list of (H, W, 3) uint8 images")
            if len(labels) != len(images):
                raise ValueError("one label array per image")
            batch, packed = None, iop.pack_ragged(list(images))
            shapes = [(h, w) for h, w, _ in packed.shapes]
        else:
            if not (torch.is_tensor(images) and images.is_cuda and images.dtype == torch.uint8 and images.dim() == 4 and images.shape[3] == 3):
                raise TypeError("augment_batch takes a list of (H, W, 3) uint8 images or a (B, H, W, 3) CUDA uint8 batch")
            if len(labels) != images.shape[0]:
                raise ValueError("one label array per image")
            batch, packed = images, None
            shapes = [(int(images.shape[1]), int(images.shape[2]))] * int(images.shape[0])
        B = len(shapes)
        if seeds is not None and len(seeds) != B:
            raise ValueError("one seed per image")
        self._sync_formats()
        angles = self.random_rotate.angles
        if seeds is not None:
            params = self._device_params(labels, shapes=shapes) if B else None
            if params is not None:
                rnd = random.Random()
                turns = np.empty((B,), dtype=np.int32)
                for i, s in enumerate(seeds):
                    rnd.seed(int(s))
                    turns[i] = rnd.choice(angles) // 90
                out, out_labels, mt_out, _ = self._augment_batch_device(batch, packed, shapes, labels, params, _seed_states(seeds), turns)
            else:
                saved, saved_py = np.random.get_state(), random.getstate()
                try:
                    try:
                        out, out_labels, mt_out = self._augment_batch_host(batch, packed, shapes, labels, seeds)
                    except NotImplementedError:
                        out, out_labels, mt_out = self._augment_batch_loop(images, labels, seeds)
                finally:
                    np.random.set_state(saved)
                    random.setstate(saved_py)
            self.__dict__["_last_generator_states"] = mt_out
            return out, out_labels
        if os.environ.get("SSDHIP_AUG_HOST_STREAM", "0") != "1" and B:
            state = np.random.get_state()
            params = self._device_params(labels, generator=state[0], shapes=shapes)
            if params is not None:
                mt = np.empty((625,), dtype=np.uint32)
                mt[:624], mt[624] = state[1], state[2]
                rnd = random.Random()
                rnd.setstate(random.getstate())
                turns = np.array([rnd.choice(angles) // 90 for _ in range(B)], dtype=np.int32)
                out, out_labels, mt_out, n_rotated = self._augment_batch_device(batch, packed, shapes, labels, params, mt, turns)
                np.random.set_state((state[0], mt_out[:624], int(mt_out[624]), state[3], state[4]))   # the stream goes on behind the batch
                for _ in range(n_rotated):                                                           # ... and so does Python's
                    random.choice(angles)
                return out, out_labels
        saved, saved_py = np.random.get_state(), random.getstate()
        try:
            out, out_labels, _ = self._augment_batch_host(batch, packed, shapes, labels, None)
        except NotImplementedError:
            np.random.set_state(saved)
            random.setstate(saved_py)
            out, out_labels, _ = self._augment_batch_loop(images, labels, None)
        return out, out_labels
