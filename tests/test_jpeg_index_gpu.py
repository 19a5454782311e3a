"""The entry-point index of the device JPEG decoder on the GPU: `decode_jpeg_batch(files, index=...)` cold (recording) and warm
(one lane per MCU row) against PIL, bit for bit; a stale index entry; and a `DataGenerator` with `decode` = 'device' over two epochs,
the second one served from `generator.jpeg_index`, against 'host'."""
import numpy as np
import pytest

from tests import np_jpeg

pytestmark = pytest.mark.gpu


def _equal(got, want):
    import torch
    assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.uint8, type(got)
    host = got.cpu().numpy()
    return host.shape == want.shape and np.array_equal(host, want)


def _delta(before, after):
    return {k: after[k] - before[k] for k in after}


def test_cold_and_warm_calls_equal_pil():
    from ssd_keras_amd.data_generator import jpeg_decode
    files = [np_jpeg.make_jpeg(375, 500, 2, 75, seed=21), np_jpeg.make_jpeg(375, 500, 0, 90, seed=22),
             np_jpeg.make_jpeg(64, 200, "L", 75, seed=24), np_jpeg.make_jpeg(17, 23, seed=4), np_jpeg.make_jpeg(1, 1, seed=1),
             np_jpeg.make_jpeg(33, 50, 0, 90, restart=2, seed=32), np_jpeg.make_jpeg(30, 44, 2, 80, seed=40, progressive=True)]
    plans = [jpeg_decode.plan_jpeg(d) for d in files]
    assert plans[6] is None and plans[5].restart_interval and all(p.restart_interval == 0 for p in plans[:5])
    assert [p.mcuy for p in plans[:5]] == [24, 47, 8, 3, 1]
    want = [np_jpeg.pil_decode(d) for d in files]
    ix = jpeg_decode.JpegIndex()
    for call, counted in enumerate(("recorded", "indexed")):
        before = dict(jpeg_decode.COUNTERS)
        got = jpeg_decode.decode_jpeg_batch(files, index=ix)
        for k, (g, w) in enumerate(zip(got[:6], want)):
            assert _equal(g, w), (call, k)
        assert isinstance(got[6], np.ndarray) and np.array_equal(got[6], want[6])
        d = _delta(before, jpeg_decode.COUNTERS)
        assert d[counted] == 4 and d["recorded"] + d["indexed"] == 4 and d["device"] == 6 and d["host"] == 1, (call, d)
        assert len(ix) == 4
    for data, plan in zip(files[:4], plans[:4]):
        rows = ix[jpeg_decode.JpegIndex.key(data, data)]
        assert rows.dtype == np.int32 and rows.shape == (plan.mcuy, 8)
        assert np.array_equal(rows[:, 3], np.arange(plan.mcuy) * plan.mcux) and tuple(rows[0]) == (0, 0, 0, 0, plan.mcux, 0, 0, 0)


def test_a_stale_entry_is_rejected_and_replaced():
    """Another image of the same size and pixel format under the old entry: the lanes notice, the file is decoded again by the
    recording route in the same call, and the result is PIL's for the NEW bytes."""
    from ssd_keras_amd.data_generator import jpeg_decode
    old, new = np_jpeg.make_jpeg(120, 160, 2, 75, seed=61), np_jpeg.make_jpeg(120, 160, 2, 75, seed=62)
    other = np_jpeg.make_jpeg(64, 96, 0, 85, seed=63)
    ix = jpeg_decode.JpegIndex()
    jpeg_decode.decode_jpeg_batch([old, other], index=ix)
    key_old, key_new, key_other = (jpeg_decode.JpegIndex.key(d, d) for d in (old, new, other))
    stale = ix.pop(key_old).copy()
    ix[key_new] = stale
    rows_other = ix[key_other].copy()
    before = dict(jpeg_decode.COUNTERS)
    got = jpeg_decode.decode_jpeg_batch([new, other], index=ix)
    assert _equal(got[0], np_jpeg.pil_decode(new)) and _equal(got[1], np_jpeg.pil_decode(other))
    d = _delta(before, jpeg_decode.COUNTERS)
    assert d["recorded"] == 1 and d["indexed"] == 1 and d["device"] == 2 and d["host"] == 0, d
    assert ix[key_new].shape == stale.shape and not np.array_equal(ix[key_new], stale)
    assert np.array_equal(ix[key_other], rows_other)
    fresh = jpeg_decode.JpegIndex()                              # the replaced entry is the one a cold call records
    jpeg_decode.decode_jpeg_batch([new], index=fresh)
    assert np.array_equal(fresh[key_new], ix[key_new])
    before = dict(jpeg_decode.COUNTERS)
    assert _equal(jpeg_decode.decode_jpeg_batch([new], index=ix)[0], np_jpeg.pil_decode(new))
    assert _delta(before, jpeg_decode.COUNTERS)["indexed"] == 1


LABELS = [[[1, 10, 8, 50, 40]], [[2, 20, 15, 80, 60], [1, 5, 5, 40, 30]], [[3, 8, 20, 50, 80]], [[1, 12, 12, 60, 70]],
          [[2, 30, 10, 90, 50]], [[1, 6, 9, 44, 66], [3, 20, 30, 60, 80]]]
SIZES = [(60, 84), (75, 100), (96, 64), (81, 81), (64, 96), (90, 70)]


def _run(names, decode):
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator
    from ssd_keras_amd.data_generator.object_detection_2d_geometric_ops import Resize
    from ssd_keras_amd.data_generator.object_detection_2d_photometric_ops import ConvertTo3Channels
    g = DataGenerator(filenames=list(names), labels=[np.array(l) for l in LABELS], image_ids=list(range(len(names))), verbose=False)
    g.decode = decode
    np.random.seed(123)
    gen = g.generate(batch_size=3, shuffle=True, transformations=[ConvertTo3Channels(), Resize(32, 32)],
                     returns={'processed_images', 'processed_labels', 'filenames'})
    return g, [next(gen) for _ in range(4)], np.random.get_state()       # two epochs of two batches


def test_generator_second_epoch_is_served_from_the_index(tmp_path):
    from ssd_keras_amd.data_generator import jpeg_decode
    names = []
    for k, (h, w) in enumerate(SIZES):
        names.append(str(tmp_path / ("im%d.jpg" % k)))
        with open(names[-1], "wb") as f:
            f.write(np_jpeg.make_jpeg(h, w, (2, 0, 1)[k % 3], 85, optimize=bool(k & 1), seed=70 + k))
    _, host, host_state = _run(names, 'host')
    before = dict(jpeg_decode.COUNTERS)
    g, dev, dev_state = _run(names, 'device')
    d = _delta(before, jpeg_decode.COUNTERS)
    assert d["recorded"] == 6 and d["indexed"] == 6 and d["device"] == 12 and d["host"] == 0, d
    assert len(g.jpeg_index) == 6
    assert host_state[0] == dev_state[0] and np.array_equal(host_state[1], dev_state[1]) and host_state[2:] == dev_state[2:]
    for b_dev, b_host in zip(dev, host):
        x_dev, y_dev, f_dev = b_dev
        x_host, y_host, f_host = b_host
        assert list(f_dev) == list(f_host)
        assert np.asarray(x_dev).dtype == np.asarray(x_host).dtype and np.array_equal(np.asarray(x_dev), np.asarray(x_host))
        assert len(y_dev) == len(y_host) and all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(y_dev, y_host))
    before = dict(jpeg_decode.COUNTERS)                          # build_jpeg_index on a fresh generator, then a warm first epoch
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator
    g2 = DataGenerator.with_decode('device', filenames=list(names), verbose=False)
    assert g2.build_jpeg_index(verbose=False) is g2.jpeg_index and len(g2.jpeg_index) == 6
    for k in g.jpeg_index.keys():
        assert np.array_equal(g.jpeg_index[k], g2.jpeg_index[k])
    g2.jpeg_index.save(str(tmp_path / "index.npz"))
    g3 = DataGenerator.with_decode('device', filenames=list(names), verbose=False)
    g3.jpeg_index = jpeg_decode.JpegIndex.load(str(tmp_path / "index.npz"))
    mid = dict(jpeg_decode.COUNTERS)
    assert _delta(before, mid)["recorded"] == 6
    g3.build_jpeg_index(verbose=False)
    d = _delta(mid, jpeg_decode.COUNTERS)
    assert d["indexed"] == 6 and d["recorded"] == 0, d
