"""Transformation lists for generate()'s 'program' path (tests/test_program_path_cpu.py, tests/test_program_path_gpu.py,
tools/time_program_path.py) and the generators they run on.  Every list is built from the package's single ops; `ns()` is the namespace
they come from."""
import os
import random
import types

import numpy as np

from tests import data_generator_cases as dc


def ns():
    from ssd_keras_amd.data_generator import object_detection_2d_geometric_ops as geo
    from ssd_keras_amd.data_generator import object_detection_2d_patch_sampling_ops as patch
    from ssd_keras_amd.data_generator import object_detection_2d_photometric_ops as photo
    from ssd_keras_amd.data_generator.data_augmentation_chain_constant_input_size import DataAugmentationConstantInputSize
    from ssd_keras_amd.data_generator.data_augmentation_chain_original_ssd import SSDDataAugmentation
    from ssd_keras_amd.data_generator.data_augmentation_chain_satellite import DataAugmentationSatellite
    from ssd_keras_amd.data_generator.data_augmentation_chain_variable_input_size import DataAugmentationVariableInputSize
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator
    out = types.SimpleNamespace(DataGenerator=DataGenerator, SSDDataAugmentation=SSDDataAugmentation,
                                DataAugmentationConstantInputSize=DataAugmentationConstantInputSize,
                                DataAugmentationVariableInputSize=DataAugmentationVariableInputSize,
                                DataAugmentationSatellite=DataAugmentationSatellite)
    for module in (geo, patch, photo):
        for name in dir(module):
            if isinstance(getattr(module, name), type):
                setattr(out, name, getattr(module, name))
    return out


def list_a(n, size=(30, 26)):
    """The float32 brightness / contrast -> HSV saturation / hue sequence of the SSD photometric chain from single ops, a flip, a resize."""
    return [n.ConvertTo3Channels(), n.ConvertDataType('float32'), n.RandomBrightness(lower=-32, upper=32, prob=0.5),
            n.RandomContrast(lower=0.5, upper=1.5, prob=0.5), n.ConvertDataType('uint8'), n.ConvertColor(current='RGB', to='HSV'),
            n.ConvertDataType('float32'), n.RandomSaturation(lower=0.5, upper=1.5, prob=0.5), n.RandomHue(max_delta=18, prob=0.5),
            n.ConvertDataType('uint8'), n.ConvertColor(current='HSV', to='RGB'), n.RandomFlip(dim='horizontal', prob=0.5),
            n.Resize(size[0], size[1])]


def list_b(n, size=(300, 300), equalize_prob=0.5, gamma_prob=0.5):
    """The list tools/time_program_path.py measures: every kind of first-segment step, with both table steps."""
    return [n.ConvertTo3Channels(), n.ConvertDataType('float32'), n.RandomBrightness(), n.RandomContrast(), n.ConvertDataType('uint8'),
            n.ConvertColor(current='RGB', to='HSV'), n.RandomHistogramEqualization(prob=equalize_prob),
            n.ConvertColor(current='HSV', to='RGB'), n.RandomGamma(prob=gamma_prob), n.RandomFlip(),
            n.RandomPadFixedAR(1.0), n.Resize(size[0], size[1])]


def list_c(n, size=(25, 27)):
    """A second segment through float64 (NumPy's result of uint8 + float), back to uint8."""
    return [n.ConvertTo3Channels(), n.Resize(size[0], size[1]), n.RandomBrightness(), n.ConvertDataType('uint8')]


def list_d(n, size=(30, 26)):
    """A float32 batch out."""
    return [n.ConvertTo3Channels(), n.Resize(size[0], size[1]), n.ConvertDataType('float32')]


def list_e(n):
    """No resize: images of one size only."""
    return [n.RandomChannelSwap(prob=0.5), n.RandomFlip(prob=0.5)]


def list_f(n, size=(30, 26)):
    return [n.ConvertTo3Channels(), n.RandomRotate(angles=[90, 180, 270], prob=0.7), n.Resize(size[0], size[1])]


def list_g(n, size=(25, 27)):
    """Tables in the SECOND segment (the uniform exports; 675 pixels per image: no dword grouping)."""
    return [n.ConvertTo3Channels(), n.Resize(size[0], size[1]), n.ConvertColor(current='RGB', to='HSV'), n.HistogramEqualization(),
            n.ConvertColor(current='HSV', to='RGB'), n.RandomGamma(prob=0.6), n.ConvertDataType('float32')]


def list_two_paddings(n, second_ratio=2.0, size=(30, 26)):
    """Two paddings with different background colours: what `GeoImage.window` cannot compose."""
    return [n.ConvertTo3Channels(), n.RandomPadFixedAR(1.0, background=(0, 0, 0)), n.RandomPadFixedAR(second_ratio, background=(9, 9, 9)),
            n.Resize(size[0], size[1])]


LISTS = {"a": list_a, "b": lambda n: list_b(n, (30, 26)), "c": list_c, "d": list_d, "e": list_e, "f": list_f, "g": list_g}


def fixture_generator(n):
    """The fixture dataset of tests/golden/data_generator: eight images of mixed sizes and channel counts with boxes."""
    return dc.csv_generator(n, load_images_into_memory=True, verbose=False)


def equal_generator(n):
    """The four fixture images of one size (18 x 22 x 3); the first has no boxes and is removed."""
    return n.DataGenerator(load_images_into_memory=True, filenames=[os.path.join(dc.FIXTURES, name) for name, _ in dc.EQUAL],
                           labels=dc.PLAIN_LABELS, verbose=False)


def array_generator(n, images, labels):
    """A DataGenerator over arrays in memory."""
    g = n.DataGenerator(verbose=False)
    g.images, g.labels = list(images), list(labels)
    g.filenames = ["array_%d" % i for i in range(len(images))]
    g.dataset_size = len(images)
    g.dataset_indices = np.arange(g.dataset_size, dtype=np.int32)
    return g


def mixed_arrays(seed=0, equal=False):
    """Noise images with odd pixel counts, grey and RGBA among them (3-channel images of one size when `equal`), and boxes."""
    rng = np.random.RandomState(seed)
    shapes = ([(37, 53), (41, 29, 1), (52, 35, 3), (33, 47, 4), (61, 45, 3), (31, 31, 3), (5, 3, 3), (29, 50)] if not equal
              else [(23, 19, 3)] * 5)
    images = [rng.randint(0, 256, size=s).astype(np.uint8) for s in shapes]
    labels = []
    for s in shapes:
        h, w = s[:2]
        x0, y0 = rng.randint(0, w - 2, size=2), rng.randint(0, h - 2, size=2)
        labels.append(np.stack([rng.randint(1, 4, size=2), x0, y0, x0 + rng.randint(1, w - x0), y0 + rng.randint(1, h - y0)], axis=1))
    return images, labels


def run_generate(n, make_generator, transformations, seed, n_batches=2, batch_size=8, device=None):
    """`n_batches` batches under one seed of both generators -> a flat dict: images (and their dtype), labels, inverters applied to a box
    array, and the two generators' final states."""
    np.random.seed(seed)
    random.seed(seed)
    returns = {'processed_images', 'processed_labels', 'inverse_transform'}
    gen = make_generator(n).generate(batch_size=batch_size, shuffle=False, transformations=transformations, returns=returns,
                                     keep_images_without_gt=False, device=device)
    out = {}
    for b in range(n_batches):
        images, labels, inverters = next(gen)
        if device is not None:
            assert images.is_cuda
            images = images.cpu().numpy()
        out["b%d_images" % b] = images
        out["b%d_dtype" % b] = np.array(str(images.dtype))
        out["b%d_n" % b] = np.array([len(l) for l in labels])
        out["b%d_labels" % b] = np.concatenate([np.asarray(l, dtype=np.float64).reshape(-1, 5) for l in labels])
        inv = []
        for fs in inverters:
            p = np.copy(dc.PREDICTIONS)
            for f in fs:
                p = f(p)
            inv.append(p)
        out["b%d_inverted" % b] = np.stack(inv)
        out["b%d_n_inverters" % b] = np.array([len(fs) for fs in inverters])
    st = np.random.get_state()
    out["np_state"] = np.concatenate([st[1].astype(np.int64), [int(st[2])]])
    out["py_state"] = np.array(random.getstate()[1], dtype=np.int64)
    return out
