"""Drop-in for the reference's data_generator/object_detection_2d_data_generator.py: `DataGenerator`, the class every training and
evaluation notebook gets its batches from, with the reference's parsers (CSV, Pascal VOC XML, MS COCO JSON), its pickled-dataset round
trip and its `generate()` semantics -- removal of images without ground truth, inverters, degenerate-box handling, the order of the
`returns` tuple, the reshuffle at every epoch wrap (`sklearn.utils.shuffle`, which draws from the global NumPy generator the augmentation
chains read too).

`generate()` picks how a batch is transformed from the transformation list it is given:
  * `[SSDDataAugmentation]`: the images (any sizes) go to the device as ONE ragged batch and the whole chain runs in a few launches
    (`SSDDataAugmentation.augment_batch` on a list of images);
  * `[ConvertTo3Channels, Resize]`, `[ConvertTo3Channels, RandomPadFixedAR, Resize]` (the evaluation lists): the label logic and the
    inverters are the transforms' own host code on lazy images (`_image_ops.GeoImage`), the pixels of the batch ONE gather launch over the
    ragged batch (`_image_ops.gather_batch_ragged`, 1- and 4-channel images folded to three channels in the read);
  * `[DataAugmentationConstantInputSize]` on images of one size: `DataAugmentationConstantInputSize.augment_batch`;
  * `[DataAugmentationVariableInputSize]`: like the first item, the images (any sizes) as ONE ragged batch through
    `DataAugmentationVariableInputSize.augment_batch` on the list (110 ms -> 2.1 ms per batch of 32, profiles/variable_chain_device.json);
  * `[DataAugmentationSatellite]`: the same for the chain with vertical flips and rotations by quarter turns
    (`DataAugmentationSatellite.augment_batch`; np.random AND Python's `random` end where the per-image loop leaves them);
  * any other list made of the package's own photometric ops, `Flip` / `RandomFlip`, `CropPad` / `Crop` / `Pad`, the random patch ops,
    `Rotate` / `RandomRotate` and one `Resize` / `ResizeRandomInterp` in the order photometric, geometric (the resize last), photometric
    (`_composable` has the rules): the list's own host code runs on lazy images that record the photometric steps around the recorded
    geometry (`_image_ops.ProgramImage`), and the batch is a few launches (`_image_ops.run_program_batch`): the first photometric
    segment on the ragged batch -- Gamma and HistogramEqualization as look-up-table steps of the per-image programs, the equalisation
    tables built on the device --, the ragged gather, the second segment on its output (which may end in float32 or float64).  A batch
    the lazy images cannot compose (NotImplementedError) goes through the per-image loop from the same random state;
  * with the generator's `compose_warps` attribute set (not in the reference; False by default, `generator.compose_warps = True`
    switches it on): such a list may also hold `Translate` / `RandomTranslate` / `Scale` / `RandomScale` among its geometric ops,
    e.g. `[ConvertTo3Channels, RandomTranslate, RandomScale, RandomFlip, Resize]` on images of mixed sizes.  The lazy images then
    carry an `_image_ops.StagedGeoImage`: a translation by whole pixels is a window of the index maps, the first zoom one
    cv2.warpAffine stage that the whole batch executes in ONE launch (`ssdhip_image_warp_affine_ragged_u8`) between the first
    segment and the gather.  A second zoom, or one behind a quarter turn, is the loop's, like every other NotImplementedError.
    Without the switch these lists take the per-image loop, as before;
  * anything else: the reference's per-image loop over the package's transforms.
Every path gives the per-image loop's pixels, labels, inverters and final `np.random` state.

Images are decoded by PIL on the host, as in the reference, unless the generator's `decode` attribute is 'device' (not in the
reference; `DataGenerator.with_decode('device', ...)` constructs one, `generator.decode = 'device'` switches one -- the constructor
keeps the reference's parameter list): then the files of a batch are decoded together on the device (`jpeg_decode.decode_jpeg_batch`: baseline JPEGs, bit for
bit PIL's pixels; every other file, and every file the device reports as damaged, is still PIL's).  The decoded images stay on the
device -- no download, no second upload -- when all of them were decoded there and the list takes the 'gather' path or one of the
ragged chain paths (`[SSDDataAugmentation]`, `[DataAugmentationVariableInputSize]`, `[DataAugmentationSatellite]`; for these three
every image must have three channels); in every other case (the 'constant' and 'program' paths, the per-image loop, no
transformations, a batch with a host-decoded member, grayscale images in front of a chain) they are downloaded and everything goes
on as with `decode='host'`.  'original_images' are NumPy arrays either way, and `load_images_into_memory=True` decodes the file list
on the device in chunks of `jpeg_decode.CHUNK` (256) files and keeps the same list of NumPy arrays.  A generator that decodes on the
device keeps `jpeg_index`, the entry points of its files without restart markers: the first decode of such a file records them, every
later one uses them (one lane per MCU row instead of one per file; same pixels), and `build_jpeg_index()` records them for the whole
dataset ahead of training.  HDF5 datasets are not supported (h5py is not a dependency of this package); their parameter and methods raise
`DatasetError`.  The parsers' XML reader is `xml.etree.ElementTree` (the reference uses BeautifulSoup) with the same results."""
from __future__ import annotations

import csv
import functools
import inspect
import json
import os
import pickle
import sys
import types
import warnings
from collections import defaultdict, namedtuple
from copy import deepcopy
from xml.etree import ElementTree

import numpy as np

from .object_detection_2d_image_boxes_validation_utils import BoxFilter


class DegenerateBatchError(Exception):
    '''Raised when a generated batch ends up degenerate, e.g. empty.'''
    pass


class DatasetError(Exception):
    '''Raised when anything is wrong with the dataset, in particular when batches are requested before a dataset was loaded.'''
    pass


_HDF5 = ("HDF5 datasets are not supported by this package (h5py is not one of its dependencies): parse the dataset with parse_csv / "
         "parse_xml / parse_json or pass file lists, and use save_dataset / get_dataset to keep it.")


def _progress(items, desc, verbose):
    if not verbose:
        return items
    try:
        from tqdm import tqdm
    except ImportError:                                    # the progress bar is cosmetic
        return items
    return tqdm(items, desc=desc, file=sys.stdout)


def _load_image(filename):
    from PIL import Image
    with Image.open(filename) as image:
        return np.array(image, dtype=np.uint8)


# how one batch of generate() is transformed: the batch path (None = the per-image loop), whether the 'program' path's lazy images
# record warps, whether a batch the device decoded is read where it is (`DataGenerator._route`)
_Route = namedtuple('_Route', 'path warps on_device')
_RAGGED_CHAINS = ('ssd', 'variable', 'satellite')                  # the paths whose chain reads a ragged batch of images of any sizes
_RETURNS = ('processed_images', 'encoded_labels', 'matched_anchors', 'processed_labels', 'filenames', 'image_ids', 'evaluation-neutral',
            'inverse_transform', 'original_images', 'original_labels')     # the order of the list generate() yields


@functools.lru_cache(maxsize=None)
def _kinds():
    """The classes `_batch_path` and `_composable` tell a list by, built on first use (the chain modules import this package's ops)."""
    from . import object_detection_2d_geometric_ops as geo
    from . import object_detection_2d_patch_sampling_ops as patch
    from . import object_detection_2d_photometric_ops as photo
    from .data_augmentation_chain_constant_input_size import DataAugmentationConstantInputSize
    from .data_augmentation_chain_original_ssd import SSDDataAugmentation
    from .data_augmentation_chain_satellite import DataAugmentationSatellite
    from .data_augmentation_chain_variable_input_size import DataAugmentationVariableInputSize
    fresh = (photo.ConvertColor, photo.ConvertDataType, photo.Brightness, photo.Contrast, photo.Gamma, photo.ChannelSwap, geo.Resize)
    in_place = (photo.Hue, photo.RandomHue, photo.Saturation, photo.RandomSaturation, photo.HistogramEqualization,
                photo.RandomHistogramEqualization)
    photometric = fresh[:-1] + in_place + (photo.RandomBrightness, photo.RandomContrast, photo.RandomGamma, photo.RandomChannelSwap)
    resizes = (geo.Resize, geo.ResizeRandomInterp)
    geometric = resizes + (geo.Flip, geo.RandomFlip, geo.Rotate, geo.RandomRotate, patch.CropPad, patch.Crop, patch.Pad,
                           patch.RandomPatch, patch.RandomPatchInf, patch.RandomMaxCropFixedAR, patch.RandomPadFixedAR)
    return types.SimpleNamespace(
        geo=geo, photo=photo, fresh=fresh, in_place=in_place, photometric=photometric, resizes=resizes, geometric=geometric,
        warped=geometric + (geo.Translate, geo.RandomTranslate, geo.Scale, geo.RandomScale),
        gather=([photo.ConvertTo3Channels, geo.Resize], [photo.ConvertTo3Channels, patch.RandomPadFixedAR, geo.Resize]),
        ragged_chains={SSDDataAugmentation: 'ssd', DataAugmentationVariableInputSize: 'variable', DataAugmentationSatellite: 'satellite'},
        constant=DataAugmentationConstantInputSize)


def _is_ssd_encoder(label_encoder):
    from ..ssd_encoder_decoder.ssd_input_encoder import SSDInputEncoder
    return isinstance(label_encoder, SSDInputEncoder)


class DataGenerator:
    '''Generates batches of samples and their labels indefinitely, shuffling the dataset consistently after each complete pass
    (reference :66-1220).  See the module docstring for how batches are transformed.'''

    def __init__(self,
                 load_images_into_memory=False,
                 hdf5_dataset_path=None,
                 filenames=None,
                 filenames_type='text',
                 images_dir=None,
                 labels=None,
                 image_ids=None,
                 eval_neutral=None,
                 labels_output_format=('class_id', 'xmin', 'ymin', 'xmax', 'ymax'),
                 verbose=True):
        self.labels_output_format = labels_output_format
        self.labels_format = {'class_id': labels_output_format.index('class_id'),
                              'xmin': labels_output_format.index('xmin'),
                              'ymin': labels_output_format.index('ymin'),
                              'xmax': labels_output_format.index('xmax'),
                              'ymax': labels_output_format.index('ymax')}
        self.dataset_size = 0
        self.load_images_into_memory = load_images_into_memory
        self.images = None
        self.compose_warps = False                      # not in the reference: lists with Translate / Scale as a device batch (module docstring)

        if filenames is not None:
            if isinstance(filenames, (list, tuple)):
                self.filenames = filenames
            elif isinstance(filenames, str):
                with open(filenames, 'rb') as f:
                    if filenames_type == 'pickle':
                        self.filenames = pickle.load(f)
                    elif filenames_type == 'text':
                        self.filenames = [os.path.join(images_dir, line.strip().decode()) for line in f]
                    else:
                        raise ValueError("`filenames_type` can be either 'text' or 'pickle'.")
            else:
                raise ValueError("`filenames` must be either a Python list/tuple or a string representing a filepath (to a pickled or text "
                                 "file). The value you passed is neither of the two.")
            self.dataset_size = len(self.filenames)
            self.dataset_indices = np.arange(self.dataset_size, dtype=np.int32)
            if load_images_into_memory:
                self.images = self._load_all(verbose)
        else:
            self.filenames = None

        self.labels = self._list_or_pickle(labels, "labels")
        self.image_ids = self._list_or_pickle(image_ids, "image_ids")
        self.eval_neutral = self._list_or_pickle(eval_neutral, "image_ids")

        self.hdf5_dataset = None
        if hdf5_dataset_path is not None:
            self.hdf5_dataset_path = hdf5_dataset_path
            self.load_hdf5_dataset(verbose=verbose)

    _decode = 'host'

    @property
    def decode(self):
        '''Who decodes the image files: 'host' (PIL, as in the reference; the default) or 'device' (baseline JPEGs on the GPU,
        `jpeg_decode.decode_jpeg_batch`; see the module docstring).  Not in the reference.'''
        return self._decode

    @decode.setter
    def decode(self, value):
        if not isinstance(value, str) or value not in ('host', 'device'):
            raise ValueError("`decode` can be either 'host' (PIL, as in the reference) or 'device' (baseline JPEGs on the GPU).")
        self._decode = value

    _jpeg_index = None

    @property
    def jpeg_index(self):
        '''The `jpeg_decode.JpegIndex` of this generator's files (decode = 'device'): entry points of the JPEGs without restart
        markers, recorded the first time a file is decoded and used from then on (`generate()`, `load_images_into_memory`,
        `build_jpeg_index`).  Assign a loaded one (`JpegIndex.load(path)`) to start warm; the device verifies every entry it
        uses, so a stale one costs time only.  Not in the reference.'''
        if self._jpeg_index is None:
            from . import jpeg_decode
            self._jpeg_index = jpeg_decode.JpegIndex()
        return self._jpeg_index

    @jpeg_index.setter
    def jpeg_index(self, value):
        self._jpeg_index = value

    def build_jpeg_index(self, verbose=True):
        '''Decode every file of the dataset once on the device, `jpeg_decode.CHUNK` files per call, so that `jpeg_index` holds
        their entry points before training starts; the images themselves are dropped.  Returns the index.  Not in the reference.'''
        from . import jpeg_decode
        if self.filenames is None:
            raise DatasetError("`build_jpeg_index()` needs the dataset's file names.")
        index = self.jpeg_index
        for start in _progress(range(0, len(self.filenames), jpeg_decode.CHUNK), 'Indexing JPEG files', verbose):
            jpeg_decode.decode_jpeg_batch(self.filenames[start:start + jpeg_decode.CHUNK], index=index)
        return index

    @classmethod
    def with_decode(cls, decode, *args, **kwargs):
        '''`DataGenerator(*args, **kwargs)` with `decode` set BEFORE the constructor runs, so that `load_images_into_memory=True`
        already decodes as asked.  The constructor itself keeps the reference's parameters.'''
        self = cls.__new__(cls)
        self.decode = decode
        self.__init__(*args, **kwargs)
        return self

    @staticmethod
    def _list_or_pickle(value, name):
        if value is None:
            return None
        if isinstance(value, str):
            with open(value, 'rb') as f:
                return pickle.load(f)
        if isinstance(value, (list, tuple)):
            return value
        raise ValueError("`{}` must be either a Python list/tuple or a string representing the path to a pickled file containing a "
                         "list/tuple. The value you passed is neither of the two.".format(name))

    def _load_images(self, verbose):
        self.dataset_size = len(self.filenames)
        self.dataset_indices = np.arange(self.dataset_size, dtype=np.int32)
        if self.load_images_into_memory:
            self.images = self._load_all(verbose)

    def _load_all(self, verbose):
        """Every file of the dataset as a NumPy array: PIL file by file, or (decode='device') the device decoder chunk by chunk."""
        if self.decode != 'device':
            return [_load_image(f) for f in _progress(self.filenames, 'Loading images into memory', verbose)]
        from . import jpeg_decode
        images = []
        for start in _progress(range(0, len(self.filenames), jpeg_decode.CHUNK), 'Loading images into memory', verbose):
            images += jpeg_decode.to_host(jpeg_decode.decode_jpeg_batch(self.filenames[start:start + jpeg_decode.CHUNK],
                                                                        index=self.jpeg_index))
        return images

    def load_hdf5_dataset(self, verbose=True):
        '''Reference :241-285 (h5py): not supported here.'''
        raise DatasetError(_HDF5)

    def create_hdf5_dataset(self, file_path='dataset.h5', resize=False, variable_image_size=True, verbose=True):
        '''Reference :597-740 (h5py): not supported here.'''
        raise DatasetError(_HDF5)

    # ---- parsers ---------------------------------------------------------------------------------------------------------------------
    def parse_csv(self,
                  images_dir,
                  labels_filename,
                  input_format,
                  include_classes='all',
                  random_sample=False,
                  ret=False,
                  verbose=True):
        '''Reference :287-386: one box per CSV row (a header row first), rows sorted, grouped by image name; the image id is the name up
        to its first dot.  `random_sample`: keep each image with that probability (one `np.random.uniform` draw per image).'''
        self.images_dir = images_dir
        self.labels_filename = labels_filename
        self.input_format = input_format
        self.include_classes = include_classes
        if self.labels_filename is None or self.input_format is None:
            raise ValueError("`labels_filename` and/or `input_format` have not been set yet. You need to pass them as arguments.")
        self.filenames, self.image_ids, self.labels = [], [], []

        data = []
        with open(self.labels_filename, newline='') as csvfile:
            csvread = csv.reader(csvfile, delimiter=',')
            next(csvread)
            for row in csvread:
                if self.include_classes == 'all' or int(row[self.input_format.index('class_id')].strip()) in self.include_classes:
                    box = [row[self.input_format.index('image_name')].strip()]
                    for element in self.labels_output_format:
                        box.append(int(row[self.input_format.index(element)].strip()))
                    data.append(box)
        data = sorted(data)

        def add(current_file, current_image_id, current_labels):
            if random_sample:
                p = np.random.uniform(0, 1)
                if not p >= (1 - random_sample):
                    return
            self.labels.append(np.stack(current_labels, axis=0))
            self.filenames.append(os.path.join(self.images_dir, current_file))
            self.image_ids.append(current_image_id)

        current_file = data[0][0]
        current_image_id = data[0][0].split('.')[0]
        current_labels = []
        for i, box in enumerate(data):
            if box[0] != current_file:
                add(current_file, current_image_id, current_labels)
                current_labels = []
                current_file = box[0]
                current_image_id = box[0].split('.')[0]
            current_labels.append(box[1:])
            if i == len(data) - 1:
                add(current_file, current_image_id, current_labels)

        self._load_images(verbose)
        if ret:
            return self.images, self.filenames, self.labels, self.image_ids

    def parse_xml(self,
                  images_dirs,
                  image_set_filenames,
                  annotations_dirs=[],
                  classes=['background',
                           'aeroplane', 'bicycle', 'bird', 'boat',
                           'bottle', 'bus', 'car', 'cat',
                           'chair', 'cow', 'diningtable', 'dog',
                           'horse', 'motorbike', 'person', 'pottedplant',
                           'sheep', 'sofa', 'train', 'tvmonitor'],
                  include_classes='all',
                  exclude_truncated=False,
                  exclude_difficult=False,
                  ret=False,
                  verbose=True):
        '''Reference :388-521: Pascal VOC image sets (one image id per line) and their XML annotations; `difficult` boxes are marked in
        `eval_neutral`.  Without annotation directories, `labels` and `eval_neutral` are None.'''
        self.images_dirs = images_dirs
        self.annotations_dirs = annotations_dirs
        self.image_set_filenames = image_set_filenames
        self.classes = classes
        self.include_classes = include_classes
        self.filenames, self.image_ids, self.labels, self.eval_neutral = [], [], [], []
        if not annotations_dirs:
            self.labels = None
            self.eval_neutral = None
            annotations_dirs = [None] * len(images_dirs)

        for images_dir, image_set_filename, annotations_dir in zip(images_dirs, image_set_filenames, annotations_dirs):
            with open(image_set_filename) as f:
                image_ids = [line.strip() for line in f]
                self.image_ids += image_ids
            for image_id in _progress(image_ids, "Processing image set '{}'".format(os.path.basename(image_set_filename)), verbose):
                filename = '{}'.format(image_id) + '.jpg'
                self.filenames.append(os.path.join(images_dir, filename))
                if annotations_dir is None:
                    continue
                root = ElementTree.parse(os.path.join(annotations_dir, image_id + '.xml')).getroot()
                folder = root.find('.//folder').text
                boxes, eval_neutr = [], []
                for obj in root.iter('object'):
                    class_name = obj.find('name').text
                    class_id = self.classes.index(class_name)
                    if (not self.include_classes == 'all') and (class_id not in self.include_classes):
                        continue
                    pose = obj.find('pose').text
                    truncated = int(obj.find('truncated').text)
                    if exclude_truncated and (truncated == 1):
                        continue
                    difficult = int(obj.find('difficult').text)
                    if exclude_difficult and (difficult == 1):
                        continue
                    bndbox = obj.find('bndbox')
                    item_dict = {'folder': folder, 'image_name': filename, 'image_id': image_id, 'class_name': class_name,
                                 'class_id': class_id, 'pose': pose, 'truncated': truncated, 'difficult': difficult,
                                 'xmin': int(bndbox.find('.//xmin').text), 'ymin': int(bndbox.find('.//ymin').text),
                                 'xmax': int(bndbox.find('.//xmax').text), 'ymax': int(bndbox.find('.//ymax').text)}
                    boxes.append([item_dict[item] for item in self.labels_output_format])
                    eval_neutr.append(bool(difficult))
                self.labels.append(boxes)
                self.eval_neutral.append(eval_neutr)

        self._load_images(verbose)
        if ret:
            return self.images, self.filenames, self.labels, self.image_ids, self.eval_neutral

    def parse_json(self,
                   images_dirs,
                   annotations_filenames,
                   ground_truth_available=False,
                   include_classes='all',
                   ret=False,
                   verbose=True):
        '''Reference :523-595: MS COCO annotation files; the 80 non-consecutive category ids become consecutive class ids 1..80
        (`cats_to_classes`, `classes_to_cats`, `cats_to_names`, `classes_to_names`); boxes [x, y, w, h] become corners.'''
        self.images_dirs = images_dirs
        self.annotations_filenames = annotations_filenames
        self.include_classes = include_classes
        self.filenames, self.image_ids, self.labels = [], [], []
        if not ground_truth_available:
            self.labels = None

        with open(annotations_filenames[0], 'r') as f:
            annotations = json.load(f)
        self.cats_to_names, self.classes_to_names, self.cats_to_classes, self.classes_to_cats = {}, ['background'], {}, {}
        for i, cat in enumerate(annotations['categories']):
            self.cats_to_names[cat['id']] = cat['name']
            self.classes_to_names.append(cat['name'])
            self.cats_to_classes[cat['id']] = i + 1
            self.classes_to_cats[i + 1] = cat['id']

        for images_dir, annotations_filename in zip(self.images_dirs, self.annotations_filenames):
            with open(annotations_filename, 'r') as f:
                annotations = json.load(f)
            if ground_truth_available:
                image_ids_to_annotations = defaultdict(list)
                for annotation in annotations['annotations']:
                    image_ids_to_annotations[annotation['image_id']].append(annotation)
            for img in _progress(annotations['images'], "Processing '{}'".format(os.path.basename(annotations_filename)), verbose):
                self.filenames.append(os.path.join(images_dir, img['file_name']))
                self.image_ids.append(img['id'])
                if not ground_truth_available:
                    continue
                boxes = []
                for annotation in image_ids_to_annotations[img['id']]:
                    cat_id = annotation['category_id']
                    if (not self.include_classes == 'all') and (cat_id not in self.include_classes):
                        continue
                    xmin, ymin, width, height = annotation['bbox'][:4]
                    item_dict = {'image_name': img['file_name'], 'image_id': img['id'], 'class_id': self.cats_to_classes[cat_id],
                                 'xmin': xmin, 'ymin': ymin, 'xmax': xmin + width, 'ymax': ymin + height}
                    boxes.append([item_dict[item] for item in self.labels_output_format])
                self.labels.append(boxes)

        self._load_images(verbose)
        if ret:
            return self.images, self.filenames, self.labels, self.image_ids

    # ---- batches ---------------------------------------------------------------------------------------------------------------------
    def _shuffle(self):
        import sklearn.utils
        objects_to_shuffle = [self.dataset_indices]
        for obj in (self.filenames, self.labels, self.image_ids, self.eval_neutral):
            if obj is not None:
                objects_to_shuffle.append(obj)
        shuffled_objects = sklearn.utils.shuffle(*objects_to_shuffle)
        for i in range(len(objects_to_shuffle)):
            objects_to_shuffle[i][:] = shuffled_objects[i]

    @staticmethod
    def _batch_path(transformations, images, have_labels):
        """Which batch path a transformation list takes (see the module docstring); None = the per-image loop."""
        k = _kinds()
        kinds = [type(t) for t in transformations]
        if not DataGenerator._batchable(images):
            return None
        if kinds in k.gather:
            return 'gather'
        if have_labels and len(kinds) == 1:
            if kinds[0] in k.ragged_chains:
                return k.ragged_chains[kinds[0]]
            if kinds[0] is k.constant and len({im.shape for im in images}) == 1 and images[0].ndim == 3 and images[0].shape[2] == 3:
                return 'constant'
        return 'program' if DataGenerator._composable(transformations, images) else None

    @staticmethod
    def _batchable(images):
        """What every batch path needs of a batch: uint8 images, (H, W) or (H, W, C) with C in 1 / 3 / 4."""
        if not images or any(not DataGenerator._is_uint8_image(im) for im in images):
            return False
        return not any(im.ndim not in (2, 3) or (im.ndim == 3 and im.shape[2] not in (1, 3, 4)) for im in images)

    def _batch_path_of(self, transformations, images, have_labels):
        """(`_batch_path`'s answer, whether the lazy images record warps) for images that stay what they are: `_route`'s first two."""
        return self._route(transformations, images, have_labels)[:2]

    def _route(self, transformations, images, have_labels, decoded=False):
        """A batch's `_Route`, decided once and before anything is downloaded.  `path` is `_batch_path`'s answer, or, with
        `compose_warps` set, 'program' for a list the paths above leave to the loop that is composable with Translate / Scale among
        the geometric ops (`warps`: the lazy images record them).  That needs NumPy images -- which a batch the device `decoded` will
        be by then: it is downloaded unless `on_device` says that its path reads it where it is.  The path found for the device
        tensors is used for their downloads: `_batch_path` and `_composable` may look at dtype, ndim and shape only, never at
        whether an image is a NumPy array or a CUDA tensor."""
        if not transformations:
            return _Route(None, False, False)
        path = self._batch_path(transformations, images, have_labels)
        if (path is None and self.compose_warps and self._batchable(images)
                and (decoded or all(isinstance(im, np.ndarray) for im in images)) and self._composable(transformations, images, warps=True)):
            return _Route('program', True, False)
        return _Route(path, False, self._stays_on_device(path, images))

    @staticmethod
    def _is_uint8_image(im):
        """A uint8 NumPy array, or (decode='device') a CUDA uint8 tensor."""
        if isinstance(im, np.ndarray):
            return im.dtype == np.uint8
        import torch
        return torch.is_tensor(im) and im.is_cuda and im.dtype == torch.uint8

    @staticmethod
    def _stays_on_device(path, images):
        """Whether a batch the device decoded is transformed where it is (module docstring): every image a device tensor, and a batch
        path that reads a ragged device batch."""
        if any(isinstance(im, np.ndarray) for im in images):
            return False
        return path == 'gather' or (path in _RAGGED_CHAINS and all(im.ndim == 3 and im.shape[2] == 3 for im in images))

    @staticmethod
    def _composable(transformations, images, warps=False):
        """Whether a list is built from the package's own photometric, index-geometry and patch ops in an order the lazy images can
        record (the 'program' path of the module docstring): decided from the elements' types and the images alone, before any draw.
        `warps`: `Translate` / `RandomTranslate` / `Scale` / `RandomScale` count as geometric ops too (`compose_warps`)."""
        k = _kinds()
        geo, photo, geometric = k.geo, k.photo, (k.warped if warps else k.geometric)
        kinds = [type(t) for t in transformations]
        if any(kind not in k.photometric and kind not in geometric and kind is not photo.ConvertTo3Channels for kind in kinds):
            return False
        if kinds[0] is not photo.ConvertTo3Channels and any(im.ndim != 3 or im.shape[2] != 3 for im in images):
            return False
        phase, resized, have_fresh = 0, False, False                   # phase: 0 photometric, 1 geometric, 2 photometric again
        for t, kind in zip(transformations, kinds):
            if kind is photo.ConvertTo3Channels:
                continue
            if kind in geometric:
                if phase == 2 or resized:                              # a lazy image is final after its resize
                    return False
                phase, resized = 1, kind in k.resizes
                if kind is geo.Rotate and t.angle not in (90, 180, 270):
                    return False
                if kind is geo.RandomRotate and any(a not in (90, 180, 270) for a in t.angles):
                    return False
            else:
                phase = 2 if phase else 0
                if kind is photo.ConvertColor and not t.keep_3ch:
                    return False
                if kind in k.in_place and not have_fresh:              # it would write into the dataset's own image in the loop
                    return False
            have_fresh = have_fresh or kind in k.fresh
        return True

    @staticmethod
    def _takes_inverter(transformations, want_inverters):
        """Per transform, whether `_walk` asks it for its inverter (reference :1070).  Asked once per batch, not per image,
        and not once per `generate()`: the list is the caller's."""
        return [want_inverters and 'return_inverter' in inspect.signature(transform).parameters for transform in transformations]

    @staticmethod
    def _walk(transformations, img, lab, takes_inverter, on_none=None):
        """The transforms' own host code on one image (reference :1066-1089), the one place that calls a transform: with the labels
        when the item came with any, asking for the inverter where `takes_inverter` says so -> (image, labels, inverters, the last
        applied first).  After every transform that leaves no image (None) the caller's `on_none()` is called; unless it raises,
        the next transform gets the None, as in the reference's loop."""
        inv, labelled = [], lab is not None
        for transform, takes in zip(transformations, takes_inverter):
            if labelled:
                if takes:
                    img, lab, inverter = transform(img, lab, return_inverter=True)
                    inv.append(inverter)
                else:
                    img, lab = transform(img, lab)
            else:
                if takes:
                    img, inverter = transform(img, return_inverter=True)
                    inv.append(inverter)
                else:
                    img = transform(img)
            if img is None and on_none is not None:
                on_none()
        return img, lab, inv[::-1]

    def _walk_batch(self, transformations, images, labels, want_inverters, lazy_of, execute):
        """The tail 'gather' and 'program' share: the transforms' own host code on one lazy image per item (`lazy_of(height, width)`),
        then `execute(lazies)`, the launches for the pixels -> what `_transform_batch` returns."""
        def refuse():
            raise NotImplementedError("a transform that drops the image is the per-image loop's to handle")
        takes = self._takes_inverter(transformations, want_inverters)
        lazies, out_labels, inverters = [], [], []
        for k, im in enumerate(images):
            img, lab, inv = self._walk(transformations, lazy_of(int(im.shape[0]), int(im.shape[1])), None if labels is None else labels[k],
                                       takes, refuse)
            lazies.append(img)
            out_labels.append(lab)
            inverters.append(inv)
        return execute(lazies), (None if labels is None else out_labels), inverters

    def _transform_batch(self, path, transformations, images, labels, want_inverters, warps=False):
        """The batch paths: images (uint8 NumPy; CUDA uint8 tensors for 'gather' and the ragged chains) and labels (arrays, or None) of the items that are transformed -> (CUDA (n, H, W, 3)
        batch -- uint8, or what a 'program' list ends in --, labels or None, inverters per item).  'program' raises NotImplementedError,
        with both random generators where they were, for a batch its lazy images cannot compose; `warps`: its lazy images record
        Translate / Scale too (`ProgramImage.of(..., warps=True)`)."""
        import torch
        from . import _image_ops as iop
        if path in _RAGGED_CHAINS or path == 'constant':           # a chain's own `augment_batch`; they differ in how it gets the images
            chain = transformations[0]
            if path == 'constant':
                batch = torch.from_numpy(np.stack(images)).to(torch.device('cuda', torch.cuda.current_device()))
            else:
                to_three = (chain.photometric_distortions if path == 'ssd' else chain).convert_to_3_channels
                batch = [im if (im.ndim == 3 and im.shape[2] == 3) else to_three(im) for im in images]
            out, out_labels = chain.augment_batch(batch, labels)
            return out, out_labels, [[] for _ in images]
        if path == 'gather':                                       # lazy images that record the geometry, one launch for the pixels
            return self._walk_batch(transformations, images, labels, want_inverters, iop.GeoImage.of,
                                    lambda lazies: iop.gather_batch_ragged(iop.pack_ragged(images), lazies))
        # 'program': lazy images that also record the photometric steps, then a few launches for the batch
        import random
        states = np.random.get_state(), random.getstate()
        try:
            return self._walk_batch(transformations, images, labels, want_inverters, functools.partial(iop.ProgramImage.of, warps=warps),
                                    lambda lazies: iop.run_program_batch(images, lazies))
        except NotImplementedError:
            np.random.set_state(states[0])
            random.setstate(states[1])
            raise

    def generate(self,
                 batch_size=32,
                 shuffle=True,
                 transformations=[],
                 label_encoder=None,
                 returns={'processed_images', 'encoded_labels'},
                 keep_images_without_gt=False,
                 degenerate_box_handling='remove',
                 device=None):
        '''Reference :742-1157: yields lists of the `returns` in the order 'processed_images', 'encoded_labels', 'matched_anchors',
        'processed_labels', 'filenames', 'image_ids', 'evaluation-neutral', 'inverse_transform', 'original_images', 'original_labels'.
        `device` (not in the reference): 'processed_images' is the CUDA uint8 batch on that device, not downloaded, and 'encoded_labels'
        come from `SSDInputEncoder.encode_to_device` (float64, on the device).'''
        if self.dataset_size == 0:
            raise DatasetError("Cannot generate batches because you did not load a dataset.")
        self._warn_of_impossible_returns(returns, label_encoder)
        if shuffle:
            self._shuffle()
        box_filter = (BoxFilter(check_overlap=False, check_min_area=False, check_degenerate=True, labels_format=self.labels_format)
                      if degenerate_box_handling == 'remove' else None)
        if self.labels is not None:
            for transform in transformations:
                transform.labels_format = self.labels_format
        if device is not None:
            import torch
            device = torch.device(device)

        current = 0
        while True:
            if current >= self.dataset_size:
                current = 0
                if shuffle:
                    self._shuffle()
            span = slice(current, current + batch_size)
            current += batch_size

            batch_X, batch_filenames, decoded = self._fetch(span)
            route = self._route(transformations, batch_X, self.labels is not None, decoded)
            if decoded and not route.on_device:
                from . import jpeg_decode
                batch_X = jpeg_decode.to_host(batch_X)
            batch_y = deepcopy(self.labels[span]) if self.labels is not None else None
            batch = {'processed_images': batch_X,                  # every list of the batch an item is removed from
                     'processed_labels': batch_y,
                     'filenames': batch_filenames,
                     'image_ids': self.image_ids[span] if self.image_ids is not None else None,
                     'evaluation-neutral': self.eval_neutral[span] if self.eval_neutral is not None else None,
                     'original_images': self._host_copies(batch_X) if 'original_images' in returns else None,
                     'original_labels': deepcopy(batch_y) if 'original_labels' in returns else None}

            processed, inverters, removed = self._transform(route, transformations, batch_X, batch_y, 'inverse_transform' in returns,
                                                            keep_images_without_gt, degenerate_box_handling, box_filter)
            batch['inverse_transform'] = inverters
            for j in sorted(removed, reverse=True):                # reference :1118-1128: the file names whatever they are, the
                for name, values in batch.items():                 # inverters while there are any, the others where they exist
                    if values or name == 'filenames':
                        values.pop(j)
            batch['processed_images'] = self._assemble(batch_X, processed, device)
            batch['encoded_labels'], batch['matched_anchors'] = self._encode(label_encoder, batch_y, 'matched_anchors' in returns, device)
            yield [batch[name] for name in _RETURNS if name in returns]

    def _warn_of_impossible_returns(self, returns, label_encoder):
        """Reference :886-905: the returns that will be None for want of labels, of an encoder, or of an `SSDInputEncoder`."""
        if self.labels is None:
            if any([ret in returns for ret in ['original_labels', 'processed_labels', 'encoded_labels', 'matched_anchors', 'evaluation-neutral']]):
                warnings.warn("Since no labels were given, none of 'original_labels', 'processed_labels', 'evaluation-neutral', 'encoded_labels', and 'matched_anchors' " +
                              "are possible returns, but you set `returns = {}`. The impossible returns will be `None`.".format(returns))
        elif label_encoder is None:
            if any([ret in returns for ret in ['encoded_labels', 'matched_anchors']]):
                warnings.warn("Since no label encoder was given, 'encoded_labels' and 'matched_anchors' aren't possible returns, " +
                              "but you set `returns = {}`. The impossible returns will be `None`.".format(returns))
        elif not _is_ssd_encoder(label_encoder):
            if 'matched_anchors' in returns:
                warnings.warn("`label_encoder` is not an `SSDInputEncoder` object, therefore 'matched_anchors' is not a possible return, " +
                              "but you set `returns = {}`. The impossible returns will be `None`.".format(returns))

    def _fetch(self, span):
        """The images of the batch at `span` of the dataset (reference :998-1017): from memory, decoded by PIL, or (decode='device')
        decoded on the device and still there -> (images, file names, whether the device decoded them)."""
        if self.images is not None:
            images = [self.images[i] for i in self.dataset_indices[span]]
            return images, (self.filenames[span] if self.filenames is not None else None), False
        filenames = self.filenames[span]
        if self.decode == 'device':
            from . import jpeg_decode
            return jpeg_decode.decode_jpeg_batch(filenames, index=self.jpeg_index), filenames, True
        return [_load_image(filename) for filename in filenames], filenames, False

    @staticmethod
    def _host_copies(images):
        """'original_images': NumPy arrays the transformations cannot reach (reference :1037)."""
        if any(not isinstance(im, np.ndarray) for im in images):
            from . import jpeg_decode
            return jpeg_decode.to_host(images)
        return deepcopy(images)

    def _transform(self, route, transformations, batch_X, batch_y, want_inverters, keep_images_without_gt, handling, box_filter):
        """Transforms the items of a batch in place, by the route's batch path or by the reference's per-image loop (:1050-1112) ->
        (the batch path's CUDA batch -- batch_X then holds its row numbers -- or None, the reference's list of inverters, the items
        to remove).  That list is the reference's with its quirks: one entry per item only when there are transformations (an item
        without ground truth has its [] either way), and one more [] per transform that left an item without an image."""
        have_labels = self.labels is not None
        todo, removed = [], []
        for i in range(len(batch_X)):
            if have_labels:
                batch_y[i] = np.array(batch_y[i])
                if batch_y[i].size == 0 and not keep_images_without_gt:
                    removed.append(i)
                    continue
            todo.append(i)
        entries = {i: [[]] for i in removed}                       # per item, what the reference appends to its ONE list of inverters
        processed = None
        if route.path is not None and todo:
            try:
                processed, out_labels, out_inverters = self._transform_batch(
                    route.path, transformations, [batch_X[i] for i in todo], [batch_y[i] for i in todo] if have_labels else None,
                    want_inverters, route.warps)
            except NotImplementedError:
                if route.path != 'program':
                    raise                                          # else this batch cannot be composed: the loop, from the same draws
        takes = self._takes_inverter(transformations, want_inverters) if processed is None else None
        for k, i in enumerate(todo):
            if processed is not None:
                batch_X[i], entries[i] = k, [out_inverters[k]]     # a row of `processed`
                if have_labels:
                    batch_y[i] = out_labels[k]
            elif transformations:
                entries[i] = []
                def dropped(i=i):                                  # reference :1076-1078, once per transform that leaves no image
                    removed.append(i)
                    entries[i].append([])
                batch_X[i], lab, inverters = self._walk(transformations, batch_X[i], batch_y[i] if have_labels else None, takes,
                                                        dropped if have_labels else None)
                entries[i].append(inverters)
                if have_labels:
                    batch_y[i] = lab
            self._check_degenerate(i, batch_y, handling, box_filter, keep_images_without_gt, removed)
        return processed, [entry for i in sorted(entries) for entry in entries[i]], removed

    def _encode(self, label_encoder, batch_y, want_anchors, device):
        """Reference :1146-1156 -> (encoded labels, matched anchors), None without an encoder or without labels; with `device`, an
        `SSDInputEncoder` encodes there."""
        if label_encoder is None or self.labels is None:
            return None, None
        if _is_ssd_encoder(label_encoder):
            if want_anchors:
                return label_encoder(batch_y, diagnostics=True)
            if device is not None:
                return label_encoder.encode_to_device(batch_y, device=device, want_f32=False, want_f64=True)[1], None
        return label_encoder(batch_y, diagnostics=False), None

    def _check_degenerate(self, i, batch_y, handling, box_filter, keep_images_without_gt, batch_items_to_remove):
        """Reference :774-795: degenerate boxes of item i after the transformations -> a warning, or BoxFilter removes them."""
        if self.labels is None:
            return
        xmin, ymin = self.labels_format['xmin'], self.labels_format['ymin']
        xmax, ymax = self.labels_format['xmax'], self.labels_format['ymax']
        if np.any(batch_y[i][:, xmax] - batch_y[i][:, xmin] <= 0) or np.any(batch_y[i][:, ymax] - batch_y[i][:, ymin] <= 0):
            if handling == 'warn':
                warnings.warn("Detected degenerate ground truth bounding boxes for batch item {} with bounding boxes {}, ".format(i, batch_y[i]) +
                              "i.e. bounding boxes where xmax <= xmin and/or ymax <= ymin. " +
                              "This could mean that your dataset contains degenerate ground truth boxes, or that any image transformations you may apply might " +
                              "result in degenerate ground truth boxes, or that you are parsing the ground truth in the wrong coordinate format." +
                              "Degenerate ground truth bounding boxes may lead to NaN errors during the training.")
            elif handling == 'remove':
                batch_y[i] = box_filter(batch_y[i])
                if (batch_y[i].size == 0) and not keep_images_without_gt:
                    batch_items_to_remove.append(i)

    @staticmethod
    def _assemble(batch_X, processed, device):
        """The batch as the reference's `np.array(batch_X)`, or as a CUDA tensor on `device`.  With a batch path, batch_X holds row
        numbers of `processed` (the images that survived removal).  An empty batch is the reference's DegenerateBatchError."""
        if device is not None:
            import torch
        if processed is None:
            batch = np.array(batch_X)
            if device is not None:
                batch = torch.from_numpy(np.ascontiguousarray(batch)).to(device)
        else:
            rows = list(batch_X)
            batch = processed.to(device) if device is not None else processed.cpu().numpy()
            if rows != list(range(int(batch.shape[0]))):
                batch = batch[rows] if device is None else batch[torch.as_tensor(rows, dtype=torch.long, device=batch.device)]
        if (batch.numel() if device is not None else batch.size) == 0:
            raise DegenerateBatchError("You produced an empty batch. This might be because the images in the batch vary " +
                                       "in their size and/or number of channels. Note that after all transformations " +
                                       "(if any were given) have been applied to all images in the batch, all images " +
                                       "must be homogenous in size along all axes.")
        return batch

    # ---- the dataset -----------------------------------------------------------------------------------------------------------------
    def save_dataset(self,
                     filenames_path='filenames.pkl',
                     labels_path=None,
                     image_ids_path=None,
                     eval_neutral_path=None):
        '''Reference :1159-1193: pickles the file names and, where a path is given, labels, image ids and eval_neutral.'''
        with open(filenames_path, 'wb') as f:
            pickle.dump(self.filenames, f)
        for path, value in ((labels_path, self.labels), (image_ids_path, self.image_ids), (eval_neutral_path, self.eval_neutral)):
            if path is not None:
                with open(path, 'wb') as f:
                    pickle.dump(value, f)

    def get_dataset(self):
        '''Returns (filenames, labels, image_ids, eval_neutral).'''
        return self.filenames, self.labels, self.image_ids, self.eval_neutral

    def get_dataset_size(self):
        '''Returns the number of images in the dataset.'''
        return self.dataset_size
