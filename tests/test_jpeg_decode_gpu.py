"""The device JPEG decoder on the GPU: `decode_jpeg_batch` against PIL, bit for bit, on the grid and on the sizes where the kernels
take other paths; the fallbacks (a file without a plan, a damaged file); and a `DataGenerator` with `decode` = 'device' against
'host' -- batches, labels, inverters and the final np.random state."""
import io

import numpy as np
import pytest

from tests import np_jpeg

pytestmark = pytest.mark.gpu


def _equal(got, want):
    import torch
    assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.uint8, type(got)
    host = got.cpu().numpy()
    return host.shape == want.shape and np.array_equal(host, want)


def test_grid_equals_pil_in_mixed_batches():
    from ssd_keras_amd.data_generator import jpeg_decode
    from ssd_keras_amd.data_generator._image_ops import RAGGED_ALIGN
    grid = np_jpeg.grid()
    assert len(grid) == 448
    for part in range(4):                                        # every call holds all sizes, samplings, qualities and table sets
        members = grid[part::4]
        got = jpeg_decode.decode_jpeg_batch([d for _, d in members])
        assert len(got) == len(members)
        base = min(g.data_ptr() for g in got)
        for (key, data), g in zip(members, got):
            assert _equal(g, np_jpeg.pil_decode(data)), key
            assert (g.data_ptr() - base) % RAGGED_ALIGN == 0, key


@pytest.mark.parametrize("case", ["420", "444", "many_segments", "odd_interval", "narrow"])
def test_sizes_where_the_kernels_take_other_paths(case):
    """375 x 500: more blocks than one workgroup of the block stage, the right-edge MCU at 500 = 31.25 MCUs, the bottom edge at 375.
    64 x 200 with a restart marker per block: more segments than a wave has lanes.  24 x 40 with an interval that does not divide the
    MCU count.  Chroma planes of one and two columns: the replicated (not filtered) upsampling."""
    from ssd_keras_amd.data_generator import jpeg_decode
    files = {"420": [np_jpeg.make_jpeg(375, 500, 2, 75, seed=21)],
             "444": [np_jpeg.make_jpeg(375, 500, 0, 90, seed=22)],
             "many_segments": [np_jpeg.make_jpeg(64, 200, 0, 75, restart=1, seed=23), np_jpeg.make_jpeg(64, 200, "L", 75, restart=1, seed=24)],
             "odd_interval": [np_jpeg.make_jpeg(24, 40, 2, 85, restart=4, seed=25), np_jpeg.make_jpeg(24, 40, 1, 85, restart=7, seed=26)],
             "narrow": [np_jpeg.make_jpeg(h, w, sub, 90, seed=w) for (h, w) in ((2, 3), (5, 4), (9, 5), (7, 6)) for sub in (1, 2)]}[case]
    if case == "many_segments":
        assert len(jpeg_decode.plan_jpeg(files[0]).segments) == 8 * 25 > 64
    if case == "odd_interval":
        plan = jpeg_decode.plan_jpeg(files[0])
        assert (plan.mcux * plan.mcuy) % plan.restart_interval != 0 and len(plan.segments) > 1
    for data, got in zip(files, jpeg_decode.decode_jpeg_batch(files)):
        assert _equal(got, np_jpeg.pil_decode(data)), case


def test_files_without_a_plan_are_pils(tmp_path):
    from PIL import Image
    from ssd_keras_amd.data_generator import jpeg_decode
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import _load_image
    names = []
    for k, (kw, ext) in enumerate([(dict(quality=80, subsampling=2), "jpg"), (dict(progressive=True), "jpg"), (dict(quality=95, subsampling=0), "jpg"),
                                   (dict(), "png")]):
        names.append(str(tmp_path / ("f%d.%s" % (k, ext))))
        Image.fromarray(np_jpeg.make_array(30 + k, 44, "RGB", 40 + k)).save(names[-1], **kw)
    before = dict(jpeg_decode.COUNTERS)
    got = jpeg_decode.decode_jpeg_batch(names)
    want = [_load_image(f) for f in names]
    assert [isinstance(g, np.ndarray) for g in got] == [False, True, False, True]
    for g, w in zip(got, want):
        g = g if isinstance(g, np.ndarray) else g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    assert jpeg_decode.COUNTERS["device"] - before["device"] == 2 and jpeg_decode.COUNTERS["host"] - before["host"] == 2


def test_a_truncated_file_is_reported_and_pil_has_the_last_word():
    """A file cut in the middle of its entropy-coded bytes: the kernel's outcome is a status word, its neighbours decode as ever, and
    `decode_jpeg_batch` raises what `_load_image` raises for that file."""
    from ssd_keras_amd.data_generator import jpeg_decode
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import _load_image
    good = [np_jpeg.make_jpeg(40, 56, 2, 80, seed=31), np_jpeg.make_jpeg(33, 50, 0, 90, restart=2, seed=32)]
    whole = np_jpeg.make_jpeg(48, 64, 2, 90, seed=33)
    plan = jpeg_decode.plan_jpeg(whole)
    cut = whole[:(plan.segments[0][0] + plan.segments[0][1]) // 2]
    datas = [good[0], cut, good[1]]
    plans = [jpeg_decode.plan_jpeg(d) for d in datas]
    assert all(p is not None for p in plans) and not plans[1].has_eoi
    views, status = jpeg_decode.decode_planned(plans, datas)
    assert status[0] == 0 and status[2] == 0 and status[1] != 0
    assert _equal(views[0], np_jpeg.pil_decode(good[0])) and _equal(views[2], np_jpeg.pil_decode(good[1]))
    with pytest.raises(Exception) as want:
        _load_image(io.BytesIO(cut))
    with pytest.raises(Exception) as got:
        jpeg_decode.decode_jpeg_batch(datas)
    assert type(got.value) is type(want.value) and str(got.value) == str(want.value)


# ---- DataGenerator with decode = 'device' ---------------------------------------------------------------------------------------------------
SIZES = [(60, 84), (75, 100), (96, 64), (81, 81), (64, 96), (90, 70)]
LABELS = [[[1, 10, 8, 50, 40]], [[2, 20, 15, 80, 60], [1, 5, 5, 40, 30]], [[3, 8, 20, 50, 80]], [[1, 12, 12, 60, 70]],
          [[2, 30, 10, 90, 50]], [[1, 6, 9, 44, 66], [3, 20, 30, 60, 80]]]


def _dataset(tmp_path, sizes):
    names = []
    for k, (h, w) in enumerate(sizes):
        names.append(str(tmp_path / ("im%d.jpg" % k)))
        with open(names[-1], "wb") as f:
            f.write(np_jpeg.make_jpeg(h, w, (2, 0, 1)[k % 3], 85, optimize=bool(k & 1), restart=(0, 3)[k & 1], seed=50 + k))
    return names


def _run(names, decode, transformations, returns, batches=3, **kw):
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator
    g = DataGenerator(filenames=list(names), labels=[np.array(l) for l in LABELS[:len(names)]], image_ids=list(range(len(names))),
                      verbose=False)
    g.decode = decode
    np.random.seed(123)
    gen = g.generate(batch_size=4, shuffle=True, transformations=transformations, returns=returns, **kw)
    out = [next(gen) for _ in range(batches)]                    # 4 + 2 files, then the reshuffle and 4 more
    return out, np.random.get_state()


def _same_state(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


def _same_batches(dev, host, returns):
    order = [r for r in ('processed_images', 'processed_labels', 'filenames', 'inverse_transform', 'original_images') if r in returns]
    predictions = np.array([[1, 0.9, 3.0, 4.0, 20.0, 25.0], [2, 0.5, 0.0, 0.0, 31.0, 31.0]])
    for d, h in zip(dev, host):
        for name, a, b in zip(order, d, h):
            if name == 'processed_images':
                assert np.asarray(a).dtype == np.asarray(b).dtype and np.array_equal(np.asarray(a), np.asarray(b))
            elif name == 'filenames':
                assert list(a) == list(b)
            elif name == 'inverse_transform':
                assert len(a) == len(b)
                for fa, fb in zip(a, b):
                    pa, pb = predictions.copy(), predictions.copy()
                    assert len(fa) == len(fb)
                    for f in fa:
                        pa = f(pa)
                    for f in fb:
                        pb = f(pb)
                    assert np.array_equal(pa, pb)
            else:
                assert len(a) == len(b)
                for x, y in zip(a, b):
                    assert isinstance(x, np.ndarray) and x.dtype == np.asarray(y).dtype and np.array_equal(x, np.asarray(y))


@pytest.mark.parametrize("case", ["eval", "variable", "plain"])
def test_generator_with_device_decoding_equals_host_decoding(tmp_path, case):
    from ssd_keras_amd.data_generator import jpeg_decode
    from ssd_keras_amd.data_generator.data_augmentation_chain_variable_input_size import DataAugmentationVariableInputSize
    from ssd_keras_amd.data_generator.object_detection_2d_geometric_ops import Resize
    from ssd_keras_amd.data_generator.object_detection_2d_photometric_ops import ConvertTo3Channels
    names = _dataset(tmp_path, SIZES if case != "plain" else [(48, 72)] * 6)
    if case == "eval":
        make, returns = (lambda: [ConvertTo3Channels(), Resize(32, 32)]), {'processed_images', 'processed_labels', 'filenames', 'inverse_transform'}
    elif case == "variable":
        make, returns = (lambda: [DataAugmentationVariableInputSize(40, 40)]), {'processed_images', 'processed_labels', 'filenames'}
    else:
        make, returns = (lambda: []), {'processed_images', 'processed_labels', 'filenames', 'original_images'}
    host, host_state = _run(names, 'host', make(), returns)
    before = dict(jpeg_decode.COUNTERS)
    dev, dev_state = _run(names, 'device', make(), returns)
    assert jpeg_decode.COUNTERS["device"] - before["device"] == 10 and jpeg_decode.COUNTERS["host"] == before["host"]
    if case == "plain":
        assert jpeg_decode.COUNTERS["downloaded"] - before["downloaded"] == 10      # once: 'original_images' copies the host arrays
    else:
        assert jpeg_decode.COUNTERS["downloaded"] == before["downloaded"]       # the images never left the device
    assert _same_state(dev_state, host_state)
    _same_batches(dev, host, returns)


def test_images_in_memory_are_the_same_list(tmp_path):
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator
    names = _dataset(tmp_path, SIZES)
    host = DataGenerator(load_images_into_memory=True, filenames=list(names), verbose=False)
    dev = DataGenerator.with_decode('device', load_images_into_memory=True, filenames=list(names), verbose=False)
    assert len(dev.images) == len(host.images) == 6
    for a, b in zip(dev.images, host.images):
        assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)
