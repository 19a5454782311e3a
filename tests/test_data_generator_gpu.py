"""DataGenerator and the ragged-batch kernels on the GPU: the ragged gather against the per-image ConvertTo3Channels + Resize, the ragged
SSDDataAugmentation.augment_batch against the per-image chain, generate()'s batch paths against the reference's goldens and against the
per-image loop, device outputs, degenerate-box removal, and Evaluator.predict_on_dataset end to end."""
import os
import types

import numpy as np
import pytest

from tests import data_generator_cases as dc
from tests import util


def _ns():
    from ssd_keras_amd.data_generator.data_augmentation_chain_original_ssd import SSDDataAugmentation
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator
    from ssd_keras_amd.data_generator.object_detection_2d_geometric_ops import Resize
    from ssd_keras_amd.data_generator.object_detection_2d_photometric_ops import ConvertTo3Channels
    return types.SimpleNamespace(DataGenerator=DataGenerator, SSDDataAugmentation=SSDDataAugmentation, Resize=Resize,
                                 ConvertTo3Channels=ConvertTo3Channels)


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(util.GOLDEN, "data_generator.npz")) as z:
        return {k: z[k] for k in z.files}


def _compare(got, want, prefix):
    keys = sorted(k for k in want if k.startswith(prefix))
    assert keys and sorted(k for k in got if k.startswith(prefix)) == keys
    for k in keys:
        assert got[k].shape == want[k].shape, k
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


class _Launches:
    """Counts the exports `_native.launch` enqueues (by name)."""

    def __init__(self, monkeypatch):
        from ssd_keras_amd import _native as nat
        self.names, real = [], nat.launch

        def counted(name, device, *args):
            self.names.append(name)
            return real(name, device, *args)
        monkeypatch.setattr(nat, "launch", counted)


def _mixed_images(rng):
    shapes = [(37, 53), (41, 29, 1), (52, 35, 3), (33, 47, 4), (60, 39, 3), (31, 31, 3), (45, 61, 4), (29, 50)]   # odd pixel counts
    return [rng.randint(0, 256, size=s).astype(np.uint8) for s in shapes]


@pytest.mark.gpu
@pytest.mark.parametrize("interp", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("out", [(24, 40), (300, 300)])
def test_ragged_gather_equals_per_image_resize(monkeypatch, interp, out):
    from ssd_keras_amd.data_generator import _image_ops as iop
    from ssd_keras_amd.data_generator.object_detection_2d_geometric_ops import Resize
    from ssd_keras_amd.data_generator.object_detection_2d_photometric_ops import ConvertTo3Channels
    images = _mixed_images(np.random.RandomState(interp))
    convert, resize = ConvertTo3Channels(), Resize(out[0], out[1], interpolation_mode=interp)
    want = np.stack([resize(convert(im)) for im in images])
    packed = iop.pack_ragged(images)
    lazies = [Resize(out[0], out[1], interpolation_mode=interp)(iop.GeoImage.of(im.shape[0], im.shape[1])) for im in images]
    count = _Launches(monkeypatch)
    got = iop.gather_batch_ragged(packed, lazies).cpu().numpy()
    assert count.names == ["ssdhip_image_resize_gather_ragged_u8"]
    np.testing.assert_array_equal(got, want)


@pytest.mark.gpu
def test_ragged_program_equals_uniform_program():
    """The photometric programs on a ragged batch (dword body + byte tail) == the uniform kernel on each image alone."""
    from ssd_keras_amd.data_generator import _image_ops as iop
    from ssd_keras_amd.data_generator.data_augmentation_chain_original_ssd import SSDPhotometricDistortions
    rng = np.random.RandomState(3)
    images = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in ((37, 53), (40, 30), (31, 31), (5, 3), (64, 65))]
    np.random.seed(11)
    pd = SSDPhotometricDistortions()
    programs = [pd.draw() for _ in images]
    packed = iop.run_ragged(iop.pack_ragged(images), programs)
    host = packed.data.cpu().numpy()
    table = packed.table.cpu().numpy()
    for im, steps, (off, h, w, c) in zip(images, programs, table):
        np.testing.assert_array_equal(host[off:off + h * w * c].reshape(h, w, c), iop.run(im, steps))


def _voc_like(B, seed):
    rng = np.random.RandomState(seed)
    images, labels = [], []
    for _ in range(B):
        h, w = int(rng.randint(300, 501)), int(rng.randint(300, 501))
        images.append(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8))
        n = int(rng.randint(1, 6))
        x0, y0 = rng.randint(0, w - 40, size=n), rng.randint(0, h - 40, size=n)
        x1, y1 = x0 + rng.randint(10, 40, size=n), y0 + rng.randint(10, 40, size=n)
        labels.append(np.stack([rng.randint(1, 21, size=n), x0, y0, x1, y1], axis=1).astype(np.int64))
    return images, labels


@pytest.mark.gpu
def test_ragged_augment_batch_equals_per_image_chain(monkeypatch):
    from ssd_keras_amd.data_generator.data_augmentation_chain_original_ssd import SSDDataAugmentation
    images, labels = _voc_like(32, 1)
    chain = SSDDataAugmentation(300, 300)
    np.random.seed(42)
    want = [chain(im, lab) for im, lab in zip(images, labels)]
    want_state = np.random.get_state()
    np.random.seed(42)
    count = _Launches(monkeypatch)
    got, got_labels = chain.augment_batch(images, labels)
    assert count.names == ["ssdhip_ssd_augment_decide_stream_ragged", "ssdhip_image_program_ragged_u8", "ssdhip_augment_plans_ragged",
                           "ssdhip_image_resize_gather_ragged_u8"]
    got = got.cpu().numpy()
    for i, (im, lab) in enumerate(want):
        np.testing.assert_array_equal(got[i], im, err_msg="image %d" % i)
        np.testing.assert_array_equal(got_labels[i], lab, err_msg="labels %d" % i)
        assert got_labels[i].dtype == lab.dtype
    st = np.random.get_state()
    assert np.array_equal(st[1], want_state[1]) and st[2] == want_state[2]


@pytest.mark.gpu
def test_generate_batch_paths_match_reference(golden):
    out = {}
    dc.run_ssd(_ns(), out)
    _compare(out, golden, "ssd_")
    dc.run_eval(_ns(), out)
    _compare(out, golden, "eval_")


@pytest.mark.gpu
def test_generate_batch_paths_equal_per_image_loop(monkeypatch):
    """The same calls with the batch paths switched off (the reference's per-image loop over the package's transforms)."""
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator
    fast = {}
    dc.run_ssd(_ns(), fast)
    dc.run_eval(_ns(), fast)
    monkeypatch.setattr(DataGenerator, "_batch_path", staticmethod(lambda *a: None))
    slow = {}
    dc.run_ssd(_ns(), slow)
    dc.run_eval(_ns(), slow)
    _compare(fast, slow, "ssd_")
    _compare(fast, slow, "eval_")


@pytest.mark.gpu
def test_device_outputs_equal_numpy_outputs():
    import torch
    from ssd_keras_amd.ssd_encoder_decoder.ssd_input_encoder import SSDInputEncoder
    enc = SSDInputEncoder(img_height=300, img_width=300, n_classes=3, predictor_sizes=[(10, 10), (5, 5)], scales=[0.2, 0.5, 0.8],
                          aspect_ratios_global=[1.0, 2.0, 0.5], two_boxes_for_ar1=True)
    ns = _ns()
    for transforms in ([ns.SSDDataAugmentation(300, 300)], [ns.ConvertTo3Channels(), ns.Resize(300, 300)]):
        outs = []
        for device in (None, 'cuda'):
            np.random.seed(9)
            g = dc.csv_generator(ns, load_images_into_memory=True, verbose=False)
            gen = g.generate(batch_size=5, shuffle=True, transformations=transforms, label_encoder=enc,
                             returns={'processed_images', 'encoded_labels', 'processed_labels'}, device=device)
            outs.append([next(gen) for _ in range(2)])
        for (xn, yn, ln), (xd, yd, ld) in zip(*outs):
            assert torch.is_tensor(xd) and xd.is_cuda and xd.dtype == torch.uint8
            np.testing.assert_array_equal(xd.cpu().numpy(), xn)
            np.testing.assert_array_equal(yd.cpu().numpy(), yn)
            for a, b in zip(ln, ld):
                np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
def test_degenerate_boxes_removed():
    ns = _ns()
    g = ns.DataGenerator(load_images_into_memory=True, filenames=[os.path.join(dc.FIXTURES, n) for n, _ in dc.EQUAL],
                         labels=dc.PLAIN_LABELS, verbose=False)
    X, y = next(g.generate(batch_size=4, shuffle=False, transformations=[], returns={'processed_images', 'processed_labels'},
                           degenerate_box_handling='remove'))
    assert X.shape == (3, 18, 22, 3)
    want = [np.array(v) for v in dc.PLAIN_LABELS[1:]]
    want[0] = want[0][:1]                                    # [2, 5, 5, 5, 9]: xmax == xmin
    for a, b in zip(y, want):
        np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["resize", "pad"])
def test_evaluator_predict_on_dataset(mode):
    """A stand-in model (two fixed detections in 300 x 300 input coordinates) through the generator's evaluation lists."""
    import torch
    from ssd_keras_amd.eval_utils.average_precision_evaluator import Evaluator
    g = dc.csv_generator(_ns(), load_images_into_memory=True, verbose=False)
    seen = []

    def model(batch):
        assert batch.shape[1:] == (300, 300, 3)
        seen.append(int(batch.shape[0]))
        det = torch.tensor([[1, 0.9, 30, 60, 150, 240], [2, 0.4, 0, 0, 300, 300]], dtype=torch.float32)
        return det[None].repeat(batch.shape[0], 1, 1)
    ev = Evaluator(model, n_classes=3, data_generator=g, model_mode='inference')
    results = ev.predict_on_dataset(300, 300, batch_size=3, data_generator_mode=mode, verbose=False, ret=True)
    assert sum(seen) == 8
    assert [len(r) for r in results] == [0, 8, 8, 0]
    for image_id, conf, x0, y0, x1, y1 in results[2]:           # the full-input box maps back onto (a pad of) the whole image
        h, w = {os.path.splitext(n)[0]: s[:2] for n, s in dc.IMAGES}[image_id]
        if mode == "resize":
            assert (x0, y0, x1, y1) == (0, 0, w, h)
        else:
            assert x0 <= 0 and y0 <= 0 and x1 >= w and y1 >= h
