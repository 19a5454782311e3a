"""Drop-in for the reference's data_generator/data_augmentation_chain_constant_input_size.py: `DataAugmentationConstantInputSize`, the
chain the SSD7 training notebook trains with -- photometric distortions, then random translation, zoom and horizontal flip, in one of
two orders drawn per image (`np.random.choice(2)`), for images that all have one size.

`__call__` runs the reference's list of transforms image by image; the photometric part is one pixel program per image (the ops' own
`draw()` in the reference's order, csrc/ssdhip_image.hip) and each translation / zoom is one cv2.warpAffine launch (csrc/ssdhip_warp.hip).
`augment_batch` does the same for a CUDA batch in TWO pixel launches: every image's photometric program in one, and translation, zoom
and flip of the whole batch as one warp.  The random draws, the validation of every trial and the label arithmetic of a batch run on the
device too (csrc/ssdhip_augment.hip: `ssdhip_const_augment_decide[_stream]` on NumPy's MT19937 stream -- the global one, or one per image
with `seeds=` -- and `ssdhip_const_augment_plans` for the warp's tables); what that kernel does not cover (`_device_params`) runs the
geometric ops on a lazy image (`_image_ops.WarpImage`) that only records them, so their draws, validation and label arithmetic are the
per-image chain's own code in the per-image chain's order.  Either way the results are those of the `__call__` loop, bit for bit."""
from __future__ import annotations

import numpy as np

from . import _chain_batch as cb
from . import _image_ops as iop
from ._chain_batch import _seed_states  # noqa: F401  (its home until the chains shared a module; still imported from here)
from .object_detection_2d_geometric_ops import RandomFlip, RandomScale, RandomTranslate
from .object_detection_2d_image_boxes_validation_utils import BoxFilter, ImageValidator
from .object_detection_2d_photometric_ops import (ConvertColor, ConvertDataType, ConvertTo3Channels, RandomBrightness, RandomContrast,
                                                  RandomHue, RandomSaturation)


class DataAugmentationConstantInputSize:
    '''Applies a chain of photometric and geometric image transformations (reference :26-183); suitable for constant-size images only.'''

    def __init__(self,
                 random_brightness=(-48, 48, 0.5),
                 random_contrast=(0.5, 1.8, 0.5),
                 random_saturation=(0.5, 1.8, 0.5),
                 random_hue=(18, 0.5),
                 random_flip=0.5,
                 random_translate=((0.03, 0.5), (0.03, 0.5), 0.5),
                 random_scale=(0.5, 2.0, 0.5),
                 n_trials_max=3,
                 clip_boxes=True,
                 overlap_criterion='area',
                 bounds_box_filter=(0.3, 1.0),
                 bounds_validator=(0.5, 1.0),
                 n_boxes_min=1,
                 background=(0, 0, 0),
                 labels_format={'class_id': 0, 'xmin': 1, 'ymin': 2, 'xmax': 3, 'ymax': 4}):
        if (random_scale[0] >= 1) or (random_scale[1] <= 1):
            raise ValueError("This sequence of transformations only makes sense if the minimum scaling factor is <1 and the maximum scaling factor is >1.")
        self.n_trials_max = n_trials_max
        self.clip_boxes = clip_boxes
        self.overlap_criterion = overlap_criterion
        self.bounds_box_filter = bounds_box_filter
        self.bounds_validator = bounds_validator
        self.n_boxes_min = n_boxes_min
        self.background = background
        self.labels_format = labels_format

        self.box_filter = BoxFilter(check_overlap=True, check_min_area=True, check_degenerate=True, overlap_criterion=self.overlap_criterion,
                                    overlap_bounds=self.bounds_box_filter, min_area=16, labels_format=self.labels_format)
        self.image_validator = ImageValidator(overlap_criterion=self.overlap_criterion, bounds=self.bounds_validator,
                                              n_boxes_min=self.n_boxes_min, labels_format=self.labels_format)

        self.convert_RGB_to_HSV = ConvertColor(current='RGB', to='HSV')
        self.convert_HSV_to_RGB = ConvertColor(current='HSV', to='RGB')
        self.convert_to_float32 = ConvertDataType(to='float32')
        self.convert_to_uint8 = ConvertDataType(to='uint8')
        self.convert_to_3_channels = ConvertTo3Channels()

        self.random_brightness = RandomBrightness(lower=random_brightness[0], upper=random_brightness[1], prob=random_brightness[2])
        self.random_contrast = RandomContrast(lower=random_contrast[0], upper=random_contrast[1], prob=random_contrast[2])
        self.random_saturation = RandomSaturation(lower=random_saturation[0], upper=random_saturation[1], prob=random_saturation[2])
        self.random_hue = RandomHue(max_delta=random_hue[0], prob=random_hue[1])

        self.random_flip = RandomFlip(dim='horizontal', prob=random_flip, labels_format=self.labels_format)
        self.random_translate = RandomTranslate(dy_minmax=random_translate[0], dx_minmax=random_translate[1], prob=random_translate[2],
                                                clip_boxes=self.clip_boxes, box_filter=self.box_filter, image_validator=self.image_validator,
                                                n_trials_max=self.n_trials_max, background=self.background, labels_format=self.labels_format)
        self.random_zoom_in = RandomScale(min_factor=1.0, max_factor=random_scale[1], prob=random_scale[2], clip_boxes=self.clip_boxes,
                                          box_filter=self.box_filter, image_validator=self.image_validator, n_trials_max=self.n_trials_max,
                                          background=self.background, labels_format=self.labels_format)
        self.random_zoom_out = RandomScale(min_factor=random_scale[0], max_factor=1.0, prob=random_scale[2], clip_boxes=self.clip_boxes,
                                           box_filter=self.box_filter, image_validator=self.image_validator, n_trials_max=self.n_trials_max,
                                           background=self.background, labels_format=self.labels_format)

        self.sequence1 = [self.convert_to_3_channels, self.convert_to_float32, self.random_brightness, self.random_contrast,
                          self.convert_to_uint8, self.convert_RGB_to_HSV, self.convert_to_float32, self.random_saturation, self.random_hue,
                          self.convert_to_uint8, self.convert_HSV_to_RGB, self.random_translate, self.random_zoom_in, self.random_flip]
        self.sequence2 = [self.convert_to_3_channels, self.convert_to_float32, self.random_brightness, self.convert_to_uint8,
                          self.convert_RGB_to_HSV, self.convert_to_float32, self.random_saturation, self.random_hue, self.convert_to_uint8,
                          self.convert_HSV_to_RGB, self.convert_to_float32, self.random_contrast, self.convert_to_uint8, self.random_zoom_out,
                          self.random_translate, self.random_flip]

    def _draw(self):
        """One image's sequence choice and photometric draws, in the reference's order -> (sequence, pixel program, geometric ops)."""
        hsv = lambda: ([("to_u8", 0), ("rgb2hsv", 0), ("to_f32", 0)] + self.random_saturation.draw() + self.random_hue.draw()
                       + [("to_u8", 0), ("hsv2rgb", 0)])
        if np.random.choice(2):
            steps = [("to_f32", 0)] + self.random_brightness.draw() + self.random_contrast.draw() + hsv()
            return 1, steps, (self.random_translate, self.random_zoom_in, self.random_flip)
        steps = [("to_f32", 0)] + self.random_brightness.draw() + hsv() + [("to_f32", 0)] + self.random_contrast.draw() + [("to_u8", 0)]
        return 2, steps, (self.random_zoom_out, self.random_translate, self.random_flip)

    def _sync_formats(self):
        self.random_translate.labels_format = self.labels_format
        self.random_zoom_in.labels_format = self.labels_format
        self.random_zoom_out.labels_format = self.labels_format
        self.random_flip.labels_format = self.labels_format

    def __call__(self, image, labels=None):
        self._sync_formats()
        _, steps, geometric = self._draw()
        image = iop.run(self.convert_to_3_channels(image), steps)
        if labels is not None:
            for transform in geometric:
                image, labels = transform(image, labels)
            return image, labels
        for transform in geometric:
            image = transform(image)
        return image

    def _device_params(self, labels=None, generator='MT19937', shapes=None):
        """The chain's configuration as the fields of ssdhip_const_augment_params (without the image size), or None for anything the
        decision kernel (csrc/ssdhip_augment.hip) does not cover: an overlap criterion other than 'area', `border_pixels` other than
        'half', `n_boxes_min == 'all'`, more than 64 trials (`nat.CONST_AUG_MAX_TRIALS`), a probability outside [0, 1], bounds that are
        not a pair of numbers, ops that no longer share the chain's box filter / validator / clipping / background -- and, when `labels`
        is given, label arrays that are not (n, 5), of mixed dtype, not int64 / float64 or longer than `nat.AUG_MAX_BOXES`; `generator`:
        the name of np.random's bit generator, MT19937 is the one the kernel steps; `shapes` (the images' (H, W)) does not matter here."""
        from .. import _native as nat
        tr, zin, zout, fl = self.random_translate, self.random_zoom_in, self.random_zoom_out, self.random_flip
        bf, val = self.box_filter, self.image_validator
        photo = (self.random_brightness, self.random_contrast, self.random_saturation, self.random_hue)
        number = lambda v: isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)
        pair = lambda v: isinstance(v, (list, tuple)) and len(v) == 2 and number(v[0]) and number(v[1]) and v[0] <= v[1]
        ok = (generator == 'MT19937'
              and all(op.box_filter is bf and op.image_validator is val for op in (tr, zin, zout))
              and isinstance(bf, BoxFilter) and isinstance(val, ImageValidator)
              and bf.overlap_criterion == 'area' and val.overlap_criterion == 'area'
              and bf.border_pixels == 'half' and val.border_pixels == 'half'
              and bf.check_overlap and bf.check_min_area and bf.check_degenerate and number(bf.min_area)
              and pair(bf.overlap_bounds) and pair(val.bounds)
              and val.n_boxes_min != 'all' and isinstance(val.n_boxes_min, (int, np.integer)) and val.n_boxes_min >= 1
              and all(isinstance(op.n_trials_max, (int, np.integer)) for op in (tr, zin, zout))
              and tr.n_trials_max == zin.n_trials_max == zout.n_trials_max and max(1, tr.n_trials_max) <= nat.CONST_AUG_MAX_TRIALS
              and bool(tr.clip_boxes) == bool(zin.clip_boxes) == bool(zout.clip_boxes)
              and all(number(op.prob) and 0.0 <= op.prob <= 1.0 for op in photo + (tr, zin, zout, fl))
              and fl.dim == 'horizontal' and pair(tr.dy_minmax) and pair(tr.dx_minmax) and tr.dy_minmax[0] >= 0 and tr.dx_minmax[0] >= 0
              and 0 < zin.min_factor <= zin.max_factor and 0 < zout.min_factor <= zout.max_factor
              and sorted(self.labels_format.get(k, -1) for k in ('class_id', 'xmin', 'ymin', 'xmax', 'ymax')) == [0, 1, 2, 3, 4])
        if ok:
            try:
                bgs = {tuple(int(v) for v in iop.border_value(op.background, 3)) for op in (tr, zin, zout)}
                ok = len(bgs) == 1
            except (TypeError, ValueError):
                ok = False
        if ok and labels is not None:
            ok = cb.labels_fit(labels)
        if not ok:
            return None
        return dict(photo_prob=[float(op.prob) for op in photo],
                    photo_lower=[float(op.lower) for op in photo[:3]] + [-float(self.random_hue.max_delta)],
                    photo_upper=[float(op.upper) for op in photo[:3]] + [float(self.random_hue.max_delta)],
                    translate_prob=float(tr.prob), dy_min=float(tr.dy_minmax[0]), dy_max=float(tr.dy_minmax[1]),
                    dx_min=float(tr.dx_minmax[0]), dx_max=float(tr.dx_minmax[1]),
                    zoom_in_prob=float(zin.prob), zoom_in_min=float(zin.min_factor), zoom_in_max=float(zin.max_factor),
                    zoom_out_prob=float(zout.prob), zoom_out_min=float(zout.min_factor), zoom_out_max=float(zout.max_factor),
                    flip_prob=float(fl.prob), n_trials=int(max(1, tr.n_trials_max)), clip_boxes=int(bool(tr.clip_boxes)),
                    n_boxes_min=int(val.n_boxes_min), validator_lower=float(val.bounds[0]), validator_upper=float(val.bounds[1]),
                    filter_lower=float(bf.overlap_bounds[0]), filter_upper=float(bf.overlap_bounds[1]), filter_min_area=float(bf.min_area))

    def _augment_batch_device(self, batch, packed, shapes, labels, params, mt):
        """The four launches behind `_device_params`: decisions (`ssdhip_const_augment_decide[_stream]`: mt (B, 625) = one generator
        state per image, (625,) = one for the batch), the photometric programs read from the device, the warp launch's tables
        (`ssdhip_const_augment_plans`) and the warp, on the CUDA batch `batch` (the chain takes no lists: `packed` is None); ONE download
        at the end.  Returns (batch, labels, generator state(s))."""
        import torch
        from .. import _native as nat
        (h, w), cols = shapes[0], cb.label_cols(self.labels_format)
        arrs, lab_in, n_in = cb.pack_labels(labels, cols)
        ops_dev, args_dev, geo_dev, fetch = nat.const_augment_decide(dict(params, img_height=h, img_width=w), mt, lab_in, n_in, batch.device)
        distorted = nat.image_program(batch.contiguous(), ops_dev, args_dev, torch.uint8)          # both sequences end in 'to_u8'
        geo5, xtab, ytab = nat.const_augment_plans(geo_dev, h, w)
        bg = cb.background_rows(self, len(shapes), batch.device, iop.border_value(self.random_translate.background, 3))
        out = nat.image_warp_affine_u8(distorted, h, w, geo5, xtab, ytab, bg)
        _, lab_out, n_out, mt_out = fetch()
        return out, cb.unpack_labels(lab_out, n_out, cols, arrs[0].dtype), mt_out

    def _augment_batch_host(self, batch, packed, shapes, labels, seeds):
        """What `_device_params` does not cover: per image the sequence choice and the photometric draws, then the sequence's geometric ops
        on a lazy image (`_image_ops.WarpImage`) -- under the image's seed when `seeds` is given -- and the pixels of the batch in two
        launches.  Returns (batch, labels, the generator state behind each image (B, 625) | None without seeds)."""
        return cb.host_batch(batch, packed, shapes, labels, seeds, lambda: self._draw()[1:], iop.WarpImage)

    def augment_batch(self, images, labels, seeds=None):
        """The chain on a device-resident batch: images (B, H, W, 3) CUDA uint8, labels a list of B label arrays -> ((B, H, W, 3) CUDA
        uint8 batch, list of B label arrays).  The pixels take TWO launches -- the photometric programs (`ssdhip_image_program`) and
        translation + zoom + flip of the whole batch (`ssdhip_image_warp_affine_u8`).

        `seeds=None`: every random draw is the one a loop of `__call__` over the batch makes on the global np.random stream, and
        np.random ends where that loop leaves it.  The draws, the validation of every trial and the label arithmetic run on the device
        (`ssdhip_const_augment_decide_stream`: one wave walks the batch on np.random's MT19937 state, which is put back afterwards);
        `SSDHIP_AUG_HOST_STREAM=1`, or a configuration `_device_params` does not cover, takes the host loop below instead -- same
        results.

        `seeds=[s_0, ...]`: image i comes out exactly as `np.random.seed(s_i); chain(image_i, labels_i)` gives it, every image on its own
        stream (`ssdhip_const_augment_decide`: one wave per image), the global generator untouched; `_last_generator_states` (B, 625)
        holds the state behind each image.  What `_device_params` does not cover runs the per-image code under each seed."""
        return cb.augment_batch(self, images, labels, seeds, lists=False)
