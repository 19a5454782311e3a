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

from . import _chain_batch as cb
from . import _image_ops as iop
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
        return cb.photo_program(self)

    def _n_taps(self, shapes):
        """Taps per output pixel the device-built tables need for images of these (H, W): eight (Lanczos-4's) unless Resize runs in
        INTER_AREA, whose true area filter takes ceil(source / output extent) + 2 of the largest possible patch -- a rotation may swap
        height and width, so both are taken as the largest side of any image."""
        return cb.patch_n_taps(self, shapes, turned=True)

    def _device_params(self, labels=None, generator='MT19937', shapes=None):
        """The chain's configuration as the fields of ssdhip_sat_augment_params (without the image size), or None for anything the
        decision kernel (csrc/ssdhip_augment.hip) does not cover: what DataAugmentationVariableInputSize._device_params lists, except
        that both flips are allowed, each with its own `dim` and probability in [0, 1] -- and `angles` that are not a non-empty list
        within {90, 180, 270}, a rotation probability outside [0, 1], label arrays that are not int64 or float64 WITH WHOLE-NUMBER
        VALUES (the closed form of Rotate's label arithmetic holds for those only); the size conditions are taken over the smaller and
        the larger side of every image, because a rotation swaps height and width."""
        rr = self.random_rotate
        flips = ((self.random_horizontal_flip, 'horizontal'), (self.random_vertical_flip, 'vertical'))
        params = cb.patch_device_params(self, flips, labels, generator, shapes, turned=True)
        ok = (params is not None and cb.is_number(rr.prob) and 0.0 <= rr.prob <= 1.0
              and isinstance(rr.angles, (list, tuple)) and len(rr.angles) > 0
              and all(cb.is_whole(a) and a in (90, 180, 270) for a in rr.angles))
        if ok and labels is not None:
            ok = all(a.dtype != np.float64 or bool(np.all(np.isfinite(a)) and np.all(a == np.floor(a)) and np.all(np.abs(a) < 2.0 ** 52))
                     for a in map(np.asarray, labels))
        if not ok:
            return None
        return dict(params, vflip_prob=float(self.random_vertical_flip.prob), rotate_prob=float(rr.prob))

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
        out, out_labels, mt_out, geo = cb.patch_device_batch(self, batch, packed, shapes, labels, params, mt, turns)
        return out, out_labels, mt_out, int(np.count_nonzero(np.asarray(geo)[:, 7]))

    def _augment_batch_host(self, batch, packed, shapes, labels, seeds):
        """What `_device_params` does not cover: per image the photometric draws, then the two flips, RandomRotate, RandomPatch and
        Resize's own code on a lazy image -- under the image's seed (both generators) when `seeds` is given -- and the pixels of the
        batch in two launches.  Raises NotImplementedError for a geometry lazy images cannot record.  Returns (batch, labels, the
        np.random state behind each image (B, 625) | None without seeds)."""
        geometric = (self.random_horizontal_flip, self.random_vertical_flip, self.random_rotate, self.random_patch, self.resize)
        return cb.host_batch(batch, packed, shapes, labels, seeds, lambda: (self._draw(), geometric), iop.GeoImage, cb.reseed_both)

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
                cb.reseed_both(int(seeds[i]))
            px, lb = self(img, lab)
            out.append(px)
            out_labels.append(lb)
            if seeds is not None:
                cb.record_np_state(states, i)
        device = images.device if torch.is_tensor(images) else None
        return nat.to_device(np.stack(out), device=device), out_labels, states

    def _turns(self, seeds, B):
        """The quarter turns of a device batch, drawn in advance as `RandomRotate` would draw its angles: image i's first
        `random.choice` under seeds[i], or (seeds None) the next B from a copy of Python's generator."""
        angles, rnd = self.random_rotate.angles, random.Random()
        turns = np.empty((B,), dtype=np.int32)
        if seeds is None:
            rnd.setstate(random.getstate())
        for i in range(B):
            if seeds is not None:
                rnd.seed(int(seeds[i]))
            turns[i] = rnd.choice(angles) // 90
        return (turns,)

    def _rotated(self, n_rotated):
        """Python's generator goes on behind a global-stream device batch: one `random.choice` per image that rotated."""
        for _ in range(n_rotated):
            random.choice(self.random_rotate.angles)

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
        return cb.augment_batch(self, images, labels, seeds, ahead=self._turns, behind=self._rotated, loop=self._augment_batch_loop,
                                python_random=True)
