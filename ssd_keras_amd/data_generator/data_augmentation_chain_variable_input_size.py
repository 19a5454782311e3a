"""Drop-in for the reference's data_generator/data_augmentation_chain_variable_input_size.py: `DataAugmentationVariableInputSize`, a
chain close to the original SSD's for images of any size -- photometric distortions, a random patch, a random horizontal flip and the
resize to the network input -- built from the package's ops.

`__call__` runs the reference's list of transforms on one image, its pixels on the GPU one op at a time.  `augment_batch` does the same
for a batch -- a list of images of any sizes (one ragged upload, `_image_ops.pack_ragged`) or a CUDA batch of one size -- in THREE pixel
launches: every image's photometric program, the tap tables of patch + flip + resize built on the device, and one gather.  The random
draws, the validation of every patch trial and the label arithmetic of the batch run on the device too (csrc/ssdhip_augment.hip:
`ssdhip_var_augment_decide[_stream[_ragged]]` on NumPy's MT19937 stream -- the global one, or one per image with `seeds=`); what that
kernel does not cover (`_device_params`) runs the ops' own host code on lazy images (`_image_ops.GeoImage`) that only record the geometry,
in the per-image chain's order.  Either way the results are those of the `__call__` loop, bit for bit.

As in the reference, `__call__` without labels reaches for a `sequence1` the class never defines and raises AttributeError (:150), and the
`background` argument never reaches RandomPatch (:114-121): what a patch adds around an image is RandomPatch's own default, black."""
from __future__ import annotations

from . import _chain_batch as cb
from . import _image_ops as iop
from .object_detection_2d_geometric_ops import RandomFlip, Resize
from .object_detection_2d_image_boxes_validation_utils import BoxFilter, ImageValidator
from .object_detection_2d_patch_sampling_ops import PatchCoordinateGenerator, RandomPatch
from .object_detection_2d_photometric_ops import (ConvertColor, ConvertDataType, ConvertTo3Channels, RandomBrightness, RandomContrast,
                                                  RandomHue, RandomSaturation)


class DataAugmentationVariableInputSize:
    '''Photometric and geometric transformations for variable-size images (reference :29-152).'''

    def __init__(self,
                 resize_height,
                 resize_width,
                 random_brightness=(-48, 48, 0.5),
                 random_contrast=(0.5, 1.8, 0.5),
                 random_saturation=(0.5, 1.8, 0.5),
                 random_hue=(18, 0.5),
                 random_flip=0.5,
                 min_scale=0.3,
                 max_scale=2.0,
                 min_aspect_ratio=0.5,
                 max_aspect_ratio=2.0,
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

        self.random_flip = RandomFlip(dim='horizontal', prob=random_flip, labels_format=self.labels_format)
        self.patch_coord_generator = PatchCoordinateGenerator(must_match='w_ar', min_scale=min_scale, max_scale=max_scale, scale_uniformly=False,
                                                              min_aspect_ratio=min_aspect_ratio, max_aspect_ratio=max_aspect_ratio)
        self.random_patch = RandomPatch(patch_coord_generator=self.patch_coord_generator, box_filter=self.box_filter_patch,
                                        image_validator=self.image_validator, n_trials_max=self.n_trials_max, clip_boxes=self.clip_boxes,
                                        prob=1.0, can_fail=False, labels_format=self.labels_format)

        self.transformations = [self.convert_to_3_channels, self.convert_to_float32, self.random_brightness, self.random_contrast,
                                self.convert_to_uint8, self.convert_RGB_to_HSV, self.convert_to_float32, self.random_saturation,
                                self.random_hue, self.convert_to_uint8, self.convert_HSV_to_RGB, self.random_patch, self.random_flip,
                                self.resize]

    def _sync_formats(self):
        self.random_patch.labels_format = self.labels_format
        self.random_flip.labels_format = self.labels_format
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
        INTER_AREA, whose true area filter takes ceil(source / output extent) + 2 of the largest possible patch."""
        return cb.patch_n_taps(self, shapes)

    def _device_params(self, labels=None, generator='MT19937', shapes=None):
        """The chain's configuration as the fields of ssdhip_var_augment_params (without the image size), or None for anything the
        decision kernel (csrc/ssdhip_augment.hip) does not cover: a `BoundGenerator` (or anything but a pair of numbers) as bounds,
        `border_pixels` other than 'half', validator and patch filter on different criteria, box filters with other checks than the
        chain's, a patch generator that is not ('w_ar', free scales and positions), `can_fail`, a vertical flip, a probability outside
        [0, 1], an interpolation code outside 0 .. 4 -- and, when `labels` is given, label arrays that are not (n, 5), of mixed dtype,
        not int64 / float64 or longer than `nat.AUG_MAX_BOXES`; `generator`: the name of np.random's bit generator, MT19937 is the one
        the kernel steps; `shapes`: the images' (H, W) -- an image narrower than 4 px, one so small that a patch could come out empty,
        or (INTER_AREA only) sizes whose tap tables would pass 64 entries are not covered."""
        return cb.patch_device_params(self, ((self.random_flip, 'horizontal'),), labels, generator, shapes)

    def _lazy_of(self, g, h, w):
        """The GeoImage of one image's recorded geometry (a row of ssdhip_var_augment_decide*'s `geometry`) over an h x w image."""
        img = iop.GeoImage.of(h, w)
        if g[0]:
            img = img.window(int(g[1]), int(g[2]), int(g[3]), int(g[4]), self.random_patch.sample_patch.background)
        if g[10]:
            img = img[:, ::-1]
        return img.resize(self.resize.out_height, self.resize.out_width, int(g[11]))

    def _augment_batch_device(self, batch, packed, shapes, labels, params, mt):
        """The four launches behind `_device_params`: decisions (mt (B, 625) = one generator state per image, (625,) = one for the
        batch), the photometric programs read from the device, the tap tables and the gather -- on the CUDA batch `batch`, or on the
        ragged batch `packed`; ONE download at the end.  Returns (batch, labels, generator state(s))."""
        return cb.patch_device_batch(self, batch, packed, shapes, labels, params, mt)[:3]

    def _augment_batch_host(self, batch, packed, shapes, labels, seeds):
        """What `_device_params` does not cover: per image the photometric draws, then RandomPatch, RandomFlip and Resize's own code on
        a lazy image -- under the image's seed when `seeds` is given -- and the pixels of the batch in two launches.  Returns (batch,
        labels, the generator state behind each image (B, 625) | None without seeds)."""
        geometric = (self.random_patch, self.random_flip, self.resize)
        return cb.host_batch(batch, packed, shapes, labels, seeds, lambda: (self._draw(), geometric), iop.GeoImage)

    def augment_batch(self, images, labels, seeds=None):
        """The chain on a batch: images a list of (H_i, W_i, 3) uint8 NumPy arrays / CUDA tensors of any sizes (they cross PCIe in one
        copy) or a (B, H, W, 3) CUDA uint8 batch, labels a list of B (n_i, 5) arrays -> ((B, resize_height, resize_width, 3) CUDA uint8
        batch, list of B label arrays in the labels' dtype and column order).

        `seeds=None`: every random draw is the one a loop of `__call__` over the batch makes on the global np.random stream, and
        np.random ends where that loop leaves it.  The draws, the validation of every patch trial and the label arithmetic run on the
        device (`ssdhip_var_augment_decide_stream[_ragged]`: one wave walks the batch on np.random's MT19937 state, which is put back
        afterwards); `SSDHIP_AUG_HOST_STREAM=1`, or anything `_device_params` does not cover, takes the ops' host code instead -- same
        results.

        `seeds=[s_0, ...]`: image i comes out exactly as `np.random.seed(s_i); chain(image_i, labels_i)` gives it, every image on its own
        stream (`ssdhip_var_augment_decide`: one wave per image), the global generator untouched, lists of mixed sizes included;
        `_last_generator_states` (B, 625) holds the state behind each image.  What `_device_params` does not cover runs the host code
        under each seed."""
        return cb.augment_batch(self, images, labels, seeds)
