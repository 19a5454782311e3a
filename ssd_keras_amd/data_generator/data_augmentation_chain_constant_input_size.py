"""Drop-in for the reference's data_generator/data_augmentation_chain_constant_input_size.py: `DataAugmentationConstantInputSize`, the
chain the SSD7 training notebook trains with -- photometric distortions, then random translation, zoom and horizontal flip, in one of
two orders drawn per image (`np.random.choice(2)`), for images that all have one size.

`__call__` runs the reference's list of transforms image by image; the photometric part is one pixel program per image (the ops' own
`draw()` in the reference's order, csrc/ssdhip_image.hip) and each translation / zoom is one cv2.warpAffine launch (csrc/ssdhip_warp.hip).
`augment_batch` does the same for a CUDA batch in TWO pixel launches: every image's photometric program in one, and translation, zoom
and flip of the whole batch as one warp -- the geometric ops run on a lazy image (`_image_ops.WarpImage`) that only records them, so
their random draws, validation and label arithmetic are the per-image chain's own code in the per-image chain's order."""
from __future__ import annotations

import numpy as np

from . import _image_ops as iop
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

    def augment_batch(self, images, labels):
        """The chain on a device-resident batch: images (B, H, W, 3) CUDA uint8, labels a list of B label arrays -> ((B, H, W, 3) CUDA
        uint8 batch, list of B label arrays).  Every random draw is made on the host in the order a loop of `__call__` over the batch
        makes it (np.random ends where that loop leaves it); the pixels take TWO launches -- the photometric programs
        (`ssdhip_image_program`) and translation + zoom + flip of the whole batch (`ssdhip_image_warp_affine_u8`)."""
        import torch
        if not (torch.is_tensor(images) and images.is_cuda and images.dtype == torch.uint8 and images.dim() == 4 and images.shape[3] == 3):
            raise TypeError("augment_batch takes a (B, H, W, 3) CUDA uint8 batch")
        if len(labels) != images.shape[0]:
            raise ValueError("one label array per image")
        self._sync_formats()
        h, w = int(images.shape[1]), int(images.shape[2])
        programs, lazies, out_labels = [], [], []
        for lab in labels:
            _, steps, geometric = self._draw()
            img = iop.WarpImage.of(h, w)
            for transform in geometric:
                img, lab = transform(img, lab)
            programs.append(steps)
            lazies.append(img)
            out_labels.append(lab)
        return iop.warp_batch(iop.run_batch(images, programs), lazies), out_labels
