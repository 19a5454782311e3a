"""Geometric image ops of the original-SSD chain -- drop-in for data_generator/object_detection_2d_geometric_ops.py:27-262
(`Resize`, `ResizeRandomInterp`, `Flip`, `RandomFlip`).

The label arithmetic, the inverters, the random draws and the return conventions are the reference's; the resampling itself
(`cv2.resize`, :70-72) runs on the GPU with the arithmetic of OpenCV's imgproc/resize.cpp for 8-bit images (round 6;
csrc/ssdhip_image.hip, plans built by `_image_ops.resize_plan`): cv::resize's dispatch over the five interpolation modes the chain draws
from -- 11-bit fixed-point coefficients with the two-stage vertical rounding (linear) or `(sum + 2^21) >> 22` (cubic, Lanczos-4), the
area-mode bilinear variant, ResizeArea / ResizeAreaFast, nearest, copy -- checked against cases worked out by hand from that source
(tests/resize_hand_cases.py; no OpenCV binary exists here to pin against).
`Translate`, `Scale`, `Rotate` and their random forms (reference :233-772) follow the reference's control flow literally -- its random
draws in its order and through its generators (`random.choice` for RandomRotate), its trial loops, validator, box filter and clipping
order; their pixels are cv2.warpAffine (INTER_LINEAR, BORDER_CONSTANT) with the fixed-point arithmetic of OpenCV 3.4 / 4.x up to 4.10's
imgproc/imgwarp.cpp (csrc/ssdhip_warp.hip, tables built by `_image_ops.warp_tables`), checked against cases worked out by hand
(tests/affine_hand_cases.py).  Rotate keeps the reference's one-pixel shift: its adjusted matrix samples one row / column outside the
image (background 0) and never samples the opposite one."""
from __future__ import annotations

import random

import numpy as np

from . import _image_ops as iop
from .object_detection_2d_image_boxes_validation_utils import BoxFilter, ImageValidator

INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA, INTER_LANCZOS4 = 0, 1, 2, 3, 4      # cv2's values

_DEFAULT_FORMAT = {'class_id': 0, 'xmin': 1, 'ymin': 2, 'xmax': 3, 'ymax': 4}


class Resize:
    def __init__(self, height, width, interpolation_mode=INTER_LINEAR, box_filter=None, labels_format=_DEFAULT_FORMAT):
        if not (isinstance(box_filter, BoxFilter) or box_filter is None):
            raise ValueError("`box_filter` must be either `None` or a `BoxFilter` object.")
        self.out_height = height
        self.out_width = width
        self.interpolation_mode = interpolation_mode
        self.box_filter = box_filter
        self.labels_format = labels_format

    def __call__(self, image, labels=None, return_inverter=False):
        img_height, img_width = image.shape[:2]
        xmin, ymin = self.labels_format['xmin'], self.labels_format['ymin']
        xmax, ymax = self.labels_format['xmax'], self.labels_format['ymax']
        out_h, out_w = self.out_height, self.out_width

        image = iop.resize(image, out_h, out_w, self.interpolation_mode)

        def inverter(labels):
            # (the reference's inverter addresses the columns one to the RIGHT of the label format's -- predictions carry a
            # confidence column after the class id, :76-78)
            labels = np.copy(labels)
            labels[:, [ymin + 1, ymax + 1]] = np.round(labels[:, [ymin + 1, ymax + 1]] * (img_height / out_h), decimals=0)
            labels[:, [xmin + 1, xmax + 1]] = np.round(labels[:, [xmin + 1, xmax + 1]] * (img_width / out_w), decimals=0)
            return labels
        inverter.step = ('scale', img_height / out_h, img_width / out_w, (xmin + 1, ymin + 1, xmax + 1, ymax + 1))

        if labels is None:
            return (image, inverter) if return_inverter else image
        labels = np.copy(labels)
        labels[:, [ymin, ymax]] = np.round(labels[:, [ymin, ymax]] * (out_h / img_height), decimals=0)
        labels[:, [xmin, xmax]] = np.round(labels[:, [xmin, xmax]] * (out_w / img_width), decimals=0)
        if self.box_filter is not None:
            self.box_filter.labels_format = self.labels_format
            labels = self.box_filter(labels=labels, image_height=out_h, image_width=out_w)
        return (image, labels, inverter) if return_inverter else (image, labels)


class ResizeRandomInterp:
    def __init__(self, height, width,
                 interpolation_modes=[INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA, INTER_LANCZOS4],
                 box_filter=None, labels_format=_DEFAULT_FORMAT):
        if not (isinstance(interpolation_modes, (list, tuple))):
            raise ValueError("`interpolation_mode` must be a list or tuple.")
        self.height = height
        self.width = width
        self.interpolation_modes = interpolation_modes
        self.box_filter = box_filter
        self.labels_format = labels_format
        self.resize = Resize(height=self.height, width=self.width, box_filter=self.box_filter, labels_format=self.labels_format)

    def __call__(self, image, labels=None, return_inverter=False):
        self.resize.interpolation_mode = np.random.choice(self.interpolation_modes)
        self.resize.labels_format = self.labels_format
        return self.resize(image, labels, return_inverter)


class Flip:
    """A view of the image and mirrored box coordinates (reference :150-200; `return_inverter` is accepted and ignored there too)."""

    def __init__(self, dim='horizontal', labels_format=_DEFAULT_FORMAT):
        if not (dim in {'horizontal', 'vertical'}):
            raise ValueError("`dim` can be one of 'horizontal' and 'vertical'.")
        self.dim = dim
        self.labels_format = labels_format

    def __call__(self, image, labels=None, return_inverter=False):
        img_height, img_width = image.shape[:2]
        xmin, ymin = self.labels_format['xmin'], self.labels_format['ymin']
        xmax, ymax = self.labels_format['xmax'], self.labels_format['ymax']
        if self.dim == 'horizontal':
            image = image[:, ::-1]
            if labels is None:
                return image
            labels = np.copy(labels)
            labels[:, [xmin, xmax]] = img_width - labels[:, [xmax, xmin]]
            return image, labels
        image = image[::-1]
        if labels is None:
            return image
        labels = np.copy(labels)
        labels[:, [ymin, ymax]] = img_height - labels[:, [ymax, ymin]]
        return image, labels


class RandomFlip:
    def __init__(self, dim='horizontal', prob=0.5, labels_format=_DEFAULT_FORMAT):
        self.dim = dim
        self.prob = prob
        self.labels_format = labels_format
        self.flip = Flip(dim=self.dim, labels_format=self.labels_format)

    def __call__(self, image, labels=None):
        if np.random.uniform(0, 1) < (1.0 - self.prob):
            return image if labels is None else (image, labels)
        self.flip.labels_format = self.labels_format
        return self.flip(image, labels)


def _transform_corners(M, labels, xmin, ymin, xmax, ymax):
    """Two opposite corners of every box through the (2, 3) matrix M, as the reference's np.dot(M, [x, y, 1]) does."""
    ones = np.ones(labels.shape[0])
    toplefts = np.array([labels[:, xmin], labels[:, ymin], ones])
    bottomrights = np.array([labels[:, xmax], labels[:, ymax], ones])
    return np.dot(M, toplefts).T, np.dot(M, bottomrights).T


def _clip(labels, xmin, ymin, xmax, ymax, img_height, img_width):
    labels[:, [ymin, ymax]] = np.clip(labels[:, [ymin, ymax]], a_min=0, a_max=img_height - 1)
    labels[:, [xmin, xmax]] = np.clip(labels[:, [xmin, xmax]], a_min=0, a_max=img_width - 1)


class Translate:
    """Translates images by whole pixels (reference :233-317): cv2.warpAffine with the float32 matrix [[1, 0, dx], [0, 1, dy]]."""

    def __init__(self, dy, dx, clip_boxes=True, box_filter=None, background=(0, 0, 0), labels_format=_DEFAULT_FORMAT):
        if not (isinstance(box_filter, BoxFilter) or box_filter is None):
            raise ValueError("`box_filter` must be either `None` or a `BoxFilter` object.")
        self.dy_rel = dy
        self.dx_rel = dx
        self.clip_boxes = clip_boxes
        self.box_filter = box_filter
        self.background = background
        self.labels_format = labels_format

    def __call__(self, image, labels=None):
        img_height, img_width = image.shape[:2]
        dy_abs = int(round(img_height * self.dy_rel))
        dx_abs = int(round(img_width * self.dx_rel))
        M = np.float32([[1, 0, dx_abs], [0, 1, dy_abs]])
        image = iop.warp_affine(image, M, (img_width, img_height), self.background)
        if labels is None:
            return image
        xmin, ymin = self.labels_format['xmin'], self.labels_format['ymin']
        xmax, ymax = self.labels_format['xmax'], self.labels_format['ymax']
        labels = np.copy(labels)
        labels[:, [xmin, xmax]] += dx_abs
        labels[:, [ymin, ymax]] += dy_abs
        if self.box_filter is not None:
            self.box_filter.labels_format = self.labels_format
            labels = self.box_filter(labels=labels, image_height=img_height, image_width=img_width)
        if self.clip_boxes:
            _clip(labels, xmin, ymin, xmax, ymax, img_height, img_width)
        return image, labels


class RandomTranslate:
    """Translates with probability `prob` by a random fraction in `dy_minmax` / `dx_minmax` either way (reference :319-447)."""

    def __init__(self, dy_minmax=(0.03, 0.3), dx_minmax=(0.03, 0.3), prob=0.5, clip_boxes=True, box_filter=None, image_validator=None,
                 n_trials_max=3, background=(0, 0, 0), labels_format=_DEFAULT_FORMAT):
        if dy_minmax[0] > dy_minmax[1]:
            raise ValueError("It must be `dy_minmax[0] <= dy_minmax[1]`.")
        if dx_minmax[0] > dx_minmax[1]:
            raise ValueError("It must be `dx_minmax[0] <= dx_minmax[1]`.")
        if dy_minmax[0] < 0 or dx_minmax[0] < 0:
            raise ValueError("It must be `dy_minmax[0] >= 0` and `dx_minmax[0] >= 0`.")
        if not (isinstance(image_validator, ImageValidator) or image_validator is None):
            raise ValueError("`image_validator` must be either `None` or an `ImageValidator` object.")
        self.dy_minmax = dy_minmax
        self.dx_minmax = dx_minmax
        self.prob = prob
        self.clip_boxes = clip_boxes
        self.box_filter = box_filter
        self.image_validator = image_validator
        self.n_trials_max = n_trials_max
        self.background = background
        self.labels_format = labels_format
        self.translate = Translate(dy=0, dx=0, clip_boxes=self.clip_boxes, box_filter=self.box_filter, background=self.background,
                                   labels_format=self.labels_format)

    def __call__(self, image, labels=None):
        p = np.random.uniform(0, 1)
        if p >= (1.0 - self.prob):
            img_height, img_width = image.shape[:2]
            xmin, ymin = self.labels_format['xmin'], self.labels_format['ymin']
            xmax, ymax = self.labels_format['xmax'], self.labels_format['ymax']
            if self.image_validator is not None:
                self.image_validator.labels_format = self.labels_format
            self.translate.labels_format = self.labels_format
            for _ in range(max(1, self.n_trials_max)):
                dy_abs = np.random.uniform(self.dy_minmax[0], self.dy_minmax[1])
                dx_abs = np.random.uniform(self.dx_minmax[0], self.dx_minmax[1])
                dy = np.random.choice([-dy_abs, dy_abs])
                dx = np.random.choice([-dx_abs, dx_abs])
                self.translate.dy_rel = dy
                self.translate.dx_rel = dx
                if (labels is None) or (self.image_validator is None):
                    return self.translate(image, labels)
                new_labels = np.copy(labels)
                new_labels[:, [ymin, ymax]] += int(round(img_height * dy))
                new_labels[:, [xmin, xmax]] += int(round(img_width * dx))
                if self.image_validator(labels=new_labels, image_height=img_height, image_width=img_width):
                    return self.translate(image, labels)
            return image if labels is None else (image, labels)
        return image if labels is None else (image, labels)


class Scale:
    """Zooms about the image centre by `factor` (reference :449-532): cv2.getRotationMatrix2D(centre, 0, factor) + cv2.warpAffine."""

    def __init__(self, factor, clip_boxes=True, box_filter=None, background=(0, 0, 0), labels_format=_DEFAULT_FORMAT):
        if factor <= 0:
            raise ValueError("It must be `factor > 0`.")
        if not (isinstance(box_filter, BoxFilter) or box_filter is None):
            raise ValueError("`box_filter` must be either `None` or a `BoxFilter` object.")
        self.factor = factor
        self.clip_boxes = clip_boxes
        self.box_filter = box_filter
        self.background = background
        self.labels_format = labels_format

    def __call__(self, image, labels=None):
        img_height, img_width = image.shape[:2]
        M = iop.rotation_matrix_2d((img_width / 2, img_height / 2), 0, self.factor)
        image = iop.warp_affine(image, M, (img_width, img_height), self.background)
        if labels is None:
            return image
        xmin, ymin = self.labels_format['xmin'], self.labels_format['ymin']
        xmax, ymax = self.labels_format['xmax'], self.labels_format['ymax']
        labels = np.copy(labels)
        new_toplefts, new_bottomrights = _transform_corners(M, labels, xmin, ymin, xmax, ymax)
        labels[:, [xmin, ymin]] = np.round(new_toplefts, decimals=0).astype(int)
        labels[:, [xmax, ymax]] = np.round(new_bottomrights, decimals=0).astype(int)
        if self.box_filter is not None:
            self.box_filter.labels_format = self.labels_format
            labels = self.box_filter(labels=labels, image_height=img_height, image_width=img_width)
        if self.clip_boxes:
            _clip(labels, xmin, ymin, xmax, ymax, img_height, img_width)
        return image, labels


class RandomScale:
    """Scales with probability `prob` by a factor drawn from [min_factor, max_factor] (reference :534-657)."""

    def __init__(self, min_factor=0.5, max_factor=1.5, prob=0.5, clip_boxes=True, box_filter=None, image_validator=None, n_trials_max=3,
                 background=(0, 0, 0), labels_format=_DEFAULT_FORMAT):
        if not (0 < min_factor <= max_factor):
            raise ValueError("It must be `0 < min_factor <= max_factor`.")
        if not (isinstance(image_validator, ImageValidator) or image_validator is None):
            raise ValueError("`image_validator` must be either `None` or an `ImageValidator` object.")
        self.min_factor = min_factor
        self.max_factor = max_factor
        self.prob = prob
        self.clip_boxes = clip_boxes
        self.box_filter = box_filter
        self.image_validator = image_validator
        self.n_trials_max = n_trials_max
        self.background = background
        self.labels_format = labels_format
        self.scale = Scale(factor=1.0, clip_boxes=self.clip_boxes, box_filter=self.box_filter, background=self.background,
                           labels_format=self.labels_format)

    def __call__(self, image, labels=None):
        p = np.random.uniform(0, 1)
        if p >= (1.0 - self.prob):
            img_height, img_width = image.shape[:2]
            xmin, ymin = self.labels_format['xmin'], self.labels_format['ymin']
            xmax, ymax = self.labels_format['xmax'], self.labels_format['ymax']
            if self.image_validator is not None:
                self.image_validator.labels_format = self.labels_format
            self.scale.labels_format = self.labels_format
            for _ in range(max(1, self.n_trials_max)):
                factor = np.random.uniform(self.min_factor, self.max_factor)
                self.scale.factor = factor
                if (labels is None) or (self.image_validator is None):
                    return self.scale(image, labels)
                M = iop.rotation_matrix_2d((img_width / 2, img_height / 2), 0, factor)
                new_toplefts, new_bottomrights = _transform_corners(M, labels, xmin, ymin, xmax, ymax)
                new_labels = np.copy(labels)
                new_labels[:, [xmin, ymin]] = np.around(new_toplefts, decimals=0).astype(int)
                new_labels[:, [xmax, ymax]] = np.around(new_bottomrights, decimals=0).astype(int)
                if self.image_validator(labels=new_labels, image_height=img_height, image_width=img_width):
                    return self.scale(image, labels)
            return image if labels is None else (image, labels)
        return image if labels is None else (image, labels)


class Rotate:
    """Rotates counter-clockwise by 90, 180 or 270 degrees (reference :659-737).  The reference's adjusted matrix is kept as it is: for
    90 degrees on a W x H image it is [[0, 1, 0], [-1, 0, W]], so output row y samples source column W - y -- row 0 comes out as the
    border value 0 and source column 0 is never sampled (likewise a row and / or a column for 180 and 270); the labels move with the
    same matrix."""

    def __init__(self, angle, labels_format=_DEFAULT_FORMAT):
        if angle not in {90, 180, 270}:
            raise ValueError("`angle` must be in the set {90, 180, 270}.")
        self.angle = angle
        self.labels_format = labels_format

    def __call__(self, image, labels=None):
        img_height, img_width = image.shape[:2]
        M = iop.rotation_matrix_2d((img_width / 2, img_height / 2), self.angle, 1)
        cos_angle = np.abs(M[0, 0])
        sin_angle = np.abs(M[0, 1])
        img_width_new = int(img_height * sin_angle + img_width * cos_angle)
        img_height_new = int(img_height * cos_angle + img_width * sin_angle)
        M[1, 2] += (img_height_new - img_height) / 2
        M[0, 2] += (img_width_new - img_width) / 2
        image = iop.warp_affine(image, M, (img_width_new, img_height_new), 0)
        if labels is None:
            return image
        xmin, ymin = self.labels_format['xmin'], self.labels_format['ymin']
        xmax, ymax = self.labels_format['xmax'], self.labels_format['ymax']
        labels = np.copy(labels)
        new_toplefts, new_bottomrights = _transform_corners(M, labels, xmin, ymin, xmax, ymax)
        labels[:, [xmin, ymin]] = np.round(new_toplefts, decimals=0).astype(int)
        labels[:, [xmax, ymax]] = np.round(new_bottomrights, decimals=0).astype(int)
        if self.angle == 90:
            labels[:, [ymax, ymin]] = labels[:, [ymin, ymax]]
        elif self.angle == 180:
            labels[:, [ymax, ymin]] = labels[:, [ymin, ymax]]
            labels[:, [xmax, xmin]] = labels[:, [xmin, xmax]]
        elif self.angle == 270:
            labels[:, [xmax, xmin]] = labels[:, [xmin, xmax]]
        return image, labels


class RandomRotate:
    """Rotates with probability `prob` by an angle drawn with Python's `random.choice` (reference :739-772)."""

    def __init__(self, angles=[90, 180, 270], prob=0.5, labels_format=_DEFAULT_FORMAT):
        for angle in angles:
            if angle not in {90, 180, 270}:
                raise ValueError("`angles` can only contain the values 90, 180, and 270.")
        self.angles = angles
        self.prob = prob
        self.labels_format = labels_format
        self.rotate = Rotate(angle=90, labels_format=self.labels_format)

    def __call__(self, image, labels=None):
        p = np.random.uniform(0, 1)
        if p >= (1.0 - self.prob):
            self.rotate.angle = random.choice(self.angles)
            self.rotate.labels_format = self.labels_format
            return self.rotate(image, labels)
        return image if labels is None else (image, labels)
