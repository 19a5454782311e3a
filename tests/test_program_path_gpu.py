"""generate()'s 'program' path on the GPU: look-up tables as program steps (op 11), the histogram of a program's prefix, the equalisation
tables built on the device, and composed lists end to end against the per-image loop -- everything bit for bit (the oracle is the existing
per-image code: `iop.run`, `iop.lut`, `iop.equalize_table`, the loop of `generate()`)."""
import numpy as np
import pytest

from tests import program_path_cases as pc

PER_IMAGE_ONLY = {"ssdhip_image_lut_u8", "ssdhip_image_hist_u8", "ssdhip_image_resize_cv_u8", "ssdhip_image_warp_affine_u8"}
BATCH = {"ssdhip_image_program_ragged_u8", "ssdhip_image_program_ragged_lut_u8", "ssdhip_image_program_hist_u8",
         "ssdhip_image_equalize_tables", "ssdhip_image_resize_gather_ragged_u8", "ssdhip_image_resize_gather_turn_ragged_u8",
         "ssdhip_image_program", "ssdhip_image_program_lut"}


class _Launches:
    """The image exports `_native.launch` enqueues, by name (generate()'s degenerate-box filter launches too: not pixel work)."""

    def __init__(self, monkeypatch):
        from ssd_keras_amd import _native as nat
        self.names, real = [], nat.launch

        def logged(name, device, *args):
            if name.startswith("ssdhip_image_"):
                self.names.append(name)
            return real(name, device, *args)
        monkeypatch.setattr(nat, "launch", logged)


def _tables(rng, b):
    return rng.randint(0, 256, size=(b, 4, 256)).astype(np.uint8)


def _lut_programs(b):
    """Per image: a look-up step for every mask / slot pairing the batch has room for, between steps that keep the state uint8."""
    masks, programs = (1, 2, 4, 7, 3, 5, 6), []
    for i in range(b):
        programs.append([("lut", (i % 4) + 4 * masks[i % 7]), ("swap", 2 + 4 * 0 + 16 * 1), ("lut", ((i + 1) % 4) + 4 * masks[(i + 3) % 7]),
                         ("rgb2hsv", 0), ("lut", ((i + 2) % 4) + 4 * masks[(i + 5) % 7])])
    return programs


def _apply_per_image(image, steps, tables):
    from ssd_keras_amd.data_generator import _image_ops as iop
    for name, arg in steps:
        image = iop.lut(image, tables[int(arg) & 3], int(arg) >> 2) if name == "lut" else iop.run(image, [(name, arg)])
    return image


@pytest.mark.gpu
def test_lut_step_on_a_ragged_batch_equals_per_image_lut():
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.data_generator import _image_ops as iop
    rng = np.random.RandomState(1)
    images = [rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8) for h, w in ((37, 53), (5, 3), (31, 31), (40, 30), (61, 45), (7, 9), (1, 1))]
    programs, tables = _lut_programs(len(images)), _tables(rng, len(images))
    enc = [iop.encode(p) for p in programs]
    packed = iop.pack_ragged(images)
    out = nat.image_program_ragged_u8(packed.data, packed.table, packed.max_pixels, np.stack([e[0] for e in enc]), np.stack([e[1] for e in enc]),
                                      nat.to_device(tables)).cpu().numpy()
    for im, steps, tab, (off, h, w, c) in zip(images, programs, tables, packed.table.cpu().numpy()):
        np.testing.assert_array_equal(out[off:off + h * w * c].reshape(h, w, c), _apply_per_image(im, steps, tab))


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(5, 3), (7, 9), (6, 10)])            # 15 and 63 pixels: one pixel per thread; 60: dword groups
@pytest.mark.parametrize("end", ["uint8", "float32", "float64"])
def test_lut_step_on_a_uniform_batch_equals_per_image_lut(size, end):
    import torch
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.data_generator import _image_ops as iop
    rng = np.random.RandomState(2)
    batch = rng.randint(0, 256, size=(7,) + size + (3,)).astype(np.uint8)
    tail = {"uint8": [], "float32": [("to_f32", 0), ("contrast", 1.25)], "float64": [("brightness", -7.5)]}[end]
    programs, tables = [p + tail for p in _lut_programs(7)], _tables(rng, 7)
    enc = [iop.encode(p) for p in programs]
    out = nat.image_program(nat.to_device(batch), np.stack([e[0] for e in enc]), np.stack([e[1] for e in enc]), getattr(torch, end),
                            nat.to_device(tables)).cpu().numpy()
    assert str(out.dtype) == end
    for i in range(7):
        np.testing.assert_array_equal(out[i], _apply_per_image(batch[i], programs[i], tables[i]))


@pytest.mark.gpu
def test_old_exports_reject_lut_steps():
    import torch
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.data_generator import _image_ops as iop
    images = [np.zeros((5, 3, 3), dtype=np.uint8)]
    ops, args = iop.encode([("hue", 3), ("lut", 4 * 7)])
    packed = iop.pack_ragged(images)
    with pytest.raises(nat.SsdHipError):
        nat.image_program_ragged_u8(packed.data, packed.table, packed.max_pixels, ops[None], args[None])
    with pytest.raises(nat.SsdHipError):
        nat.image_program(nat.to_device(images[0][None]), ops[None], args[None], torch.uint8)
    with pytest.raises(nat.SsdHipError):
        iop.run(images[0], [("lut", 4 * 7)])                            # `run` has no tables
    # a look-up step on a float state is refused by the new exports too
    ops, args = iop.encode([("to_f32", 0), ("lut", 4 * 7)])
    with pytest.raises(nat.SsdHipError):
        nat.image_program(nat.to_device(images[0][None]), ops[None], args[None], torch.float32, nat.to_device(np.zeros((1, 4, 256), np.uint8)))


def _hist_batch(rng):
    images = [rng.randint(0, 256, size=(1, 1, 3)).astype(np.uint8), np.full((9, 7, 3), 77, dtype=np.uint8),
              rng.randint(0, 256, size=(300, 300, 3)).astype(np.uint8), rng.randint(0, 256, size=(37, 53, 3)).astype(np.uint8),
              rng.randint(0, 256, size=(5, 3, 3)).astype(np.uint8)]
    table = rng.randint(0, 256, size=256).astype(np.uint8)
    programs = [[("rgb2hsv", 0), ("lut", 4 * 4)], [("hue", 30.5), ("lut", 1 + 4 * 7), ("swap", 1 + 4 * 0 + 16 * 2)],
                [("to_f32", 0), ("contrast", 1.3), ("to_u8", 0), ("rgb2hsv", 0), ("lut", 2 + 4 * 4), ("hsv2rgb", 0)],
                [("rgb2hsv", 0), ("lut", 4 * 4)], [("saturation", 1.5), ("lut", 3 + 4 * 2)]]
    stop = np.array([1, 2, 4, -1, 0], dtype=np.int32)                   # image 3 takes no part; image 4: the image itself
    channel = np.array([2, 0, 2, 2, 1], dtype=np.int32)
    luts = np.zeros((5, 4, 256), dtype=np.uint8)
    luts[1, 1] = table
    return images, programs, stop, channel, luts


def _want_hist(images, programs, stop, channel, luts):
    want = np.zeros((len(images), 256), dtype=np.int64)
    for i, (im, p) in enumerate(zip(images, programs)):
        if stop[i] >= 0:
            want[i] = np.bincount(_apply_per_image(im, p[:stop[i]], luts[i])[..., channel[i]].ravel(), minlength=256)
    return want


@pytest.mark.gpu
def test_prefix_histogram_on_a_ragged_batch():
    import torch
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.data_generator import _image_ops as iop
    images, programs, stop, channel, luts = _hist_batch(np.random.RandomState(3))
    enc = [iop.encode(p) for p in programs]
    ops, args = np.stack([e[0] for e in enc]), np.stack([e[1] for e in enc])
    packed = iop.pack_ragged(images)
    before = packed.data.clone()
    hist = torch.full((5, 256), 12345, dtype=torch.int32, device=packed.data.device)       # the export zeroes it
    want = _want_hist(images, programs, stop, channel, luts)
    for _ in range(2):                                                   # twice into the same buffer
        got = nat.image_program_hist_u8(packed.data, packed.table, packed.max_pixels, ops, args, nat.to_device(luts), stop, channel, hist)
        assert got is hist
        np.testing.assert_array_equal(hist.cpu().numpy(), want)
    assert want[2].sum() == 90000 and not want[3].any() and (want[1] > 0).sum() == 1
    assert torch.equal(packed.data, before)                             # nothing else is written


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(300, 300), (5, 3), (9, 7)])           # several workgroups per image; 15 / 63 pixels: one pixel per thread
def test_prefix_histogram_on_a_uniform_batch(size):
    import torch
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.data_generator import _image_ops as iop
    rng = np.random.RandomState(4)
    _, programs, stop, channel, luts = _hist_batch(rng)
    batch = rng.randint(0, 256, size=(5,) + size + (3,)).astype(np.uint8)
    batch[1] = 77
    enc = [iop.encode(p) for p in programs]
    dev = nat.to_device(batch)
    hist = torch.full((5, 256), -1, dtype=torch.int32, device=dev.device)
    want = _want_hist(list(batch), programs, stop, channel, luts)
    for _ in range(2):
        nat.image_program_hist_u8(dev, None, 0, np.stack([e[0] for e in enc]), np.stack([e[1] for e in enc]), nat.to_device(luts), stop, channel, hist)
        np.testing.assert_array_equal(hist.cpu().numpy(), want)


def _crafted_histograms():
    h = np.zeros((8, 256), dtype=np.int64)
    h[0, 93] = 4000                                                      # one occupied bin: the identity
    h[1, 255] = 17                                                       # ... the last one
    h[2, 10], h[2, 200] = 5, 7                                           # two bins
    h[3, 3], h[3, 7], h[3, 9], h[3, 250] = 11, 1, 2, 507                 # total - hist[first] = 510: 1 -> 0.5 -> 0, 3 -> 1.5 -> 2
    h[4] = np.random.RandomState(5).randint(0, 1000, size=256)
    h[5, 100:] = np.random.RandomState(6).randint(0, 3, size=156) * 40000
    h[6, 1] = 9                                                          # skipped (slot -1): its tables stay as they are
    h[7, 0], h[7, 255] = 1, 2 ** 31                                      # counts beyond float32's integers and int32's range
    return h


@pytest.mark.gpu
def test_equalize_tables_equal_the_host_rule():
    import torch
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.data_generator import _image_ops as iop
    h = _crafted_histograms()
    want3 = iop.equalize_table(h[3])
    assert want3[7] == 0 and want3[9] == 2 and want3[250] == 255 and want3[3] == 0     # the exact halves round to even
    slot = np.array([0, 1, 2, 3, 0, 1, -1, 2], dtype=np.int32)
    luts = nat.to_device(np.full((8, 4, 256), 201, dtype=np.uint8))
    hist = nat.to_device(h.astype(np.uint32).view(np.int32))
    assert nat.image_equalize_tables(hist, slot, luts) is luts
    got = luts.cpu().numpy()
    for i in range(8):
        for s in range(4):
            want = iop.equalize_table(h[i]) if s == slot[i] else np.full(256, 201, dtype=np.uint8)
            np.testing.assert_array_equal(got[i, s], want, err_msg="histogram %d slot %d" % (i, s))
    np.testing.assert_array_equal(got[0, 0], np.arange(256))
    np.testing.assert_array_equal(got[1, 1], np.arange(256))


def _assert_same(fast, slow):
    assert sorted(fast) == sorted(slow)
    for k in sorted(slow):
        assert fast[k].shape == slow[k].shape and fast[k].dtype == slow[k].dtype, k
        np.testing.assert_array_equal(fast[k], slow[k], err_msg=k)


def _sources(name):
    if name == "e":
        return [pc.equal_generator, lambda n: pc.array_generator(n, *pc.mixed_arrays(8, equal=True))]
    return [pc.fixture_generator, lambda n: pc.array_generator(n, *pc.mixed_arrays(7))]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(pc.LISTS))
def test_composed_lists_equal_the_per_image_loop(monkeypatch, name):
    """Lists (a) - (f) of the issue and one with tables in the second segment, on the fixture dataset and on noise arrays: pixels, dtype,
    labels, inverters and both generators' states, with and without `device=`; no batch falls back to per-image launches."""
    n = pc.ns()
    end = {"d": "float32", "g": "float32"}.get(name, "uint8")
    for k, source in enumerate(_sources(name)):
        log = _Launches(monkeypatch)
        fast = pc.run_generate(n, source, pc.LISTS[name](n), seed=20 + k)
        names = list(log.names)
        on_device = pc.run_generate(n, source, pc.LISTS[name](n), seed=20 + k, device='cuda')
        monkeypatch.undo()
        monkeypatch.setattr(n.DataGenerator, "_batch_path", staticmethod(lambda *a: None))
        slow = pc.run_generate(n, source, pc.LISTS[name](n), seed=20 + k)
        monkeypatch.undo()
        _assert_same(fast, slow)
        _assert_same(on_device, slow)
        assert str(fast["b0_dtype"]) == end
        # two batches: only batch exports, a handful of them
        assert set(names) <= BATCH and not set(names) & PER_IMAGE_ONLY, names
        assert len(names) <= 2 * 6 and names.count("ssdhip_image_program") + names.count("ssdhip_image_program_lut") <= 2, names
        if name in ("c", "d"):
            assert names == ["ssdhip_image_resize_gather_ragged_u8", "ssdhip_image_program"] * 2
        if name == "g":
            assert names == ["ssdhip_image_resize_gather_ragged_u8", "ssdhip_image_program_hist_u8", "ssdhip_image_equalize_tables",
                             "ssdhip_image_program_lut"] * 2


@pytest.mark.gpu
@pytest.mark.parametrize("equalize_prob, want", [
    (1.0, ["ssdhip_image_program_hist_u8", "ssdhip_image_equalize_tables", "ssdhip_image_program_ragged_lut_u8",
           "ssdhip_image_resize_gather_ragged_u8"]),
    (0.0, ["ssdhip_image_program_ragged_lut_u8", "ssdhip_image_resize_gather_ragged_u8"])])
def test_launches_of_the_measured_list(monkeypatch, equalize_prob, want):
    n = pc.ns()
    transformations = pc.list_b(n, (30, 26), equalize_prob=equalize_prob, gamma_prob=1.0)
    log = _Launches(monkeypatch)
    fast = pc.run_generate(n, pc.fixture_generator, transformations, seed=31, n_batches=1)
    assert log.names == want
    monkeypatch.undo()
    monkeypatch.setattr(n.DataGenerator, "_batch_path", staticmethod(lambda *a: None))
    _assert_same(fast, pc.run_generate(n, pc.fixture_generator, transformations, seed=31, n_batches=1))


@pytest.mark.gpu
@pytest.mark.parametrize("second_ratio", [2.0, 0.5])
def test_a_batch_that_cannot_be_composed_falls_back_to_the_loop(monkeypatch, second_ratio):
    """Two paddings with different backgrounds: `_batch_path` says 'program' (it decides before any draw); where the second op really
    pads a padded image (ratio 0.5: rows under the first op's columns) `GeoImage.window` raises and the batch is the loop's, from the
    same generator states.  Either way the output and the states are the loop's."""
    n = pc.ns()
    transformations = pc.list_two_paddings(n, second_ratio)
    assert n.DataGenerator._batch_path(transformations, [np.zeros((7, 9), dtype=np.uint8)], True) == 'program'
    log = _Launches(monkeypatch)
    fast = pc.run_generate(n, pc.fixture_generator, transformations, seed=41)
    names = list(log.names)
    monkeypatch.undo()
    monkeypatch.setattr(n.DataGenerator, "_batch_path", staticmethod(lambda *a: None))
    slow = pc.run_generate(n, pc.fixture_generator, transformations, seed=41)
    _assert_same(fast, slow)
    if second_ratio == 0.5:
        assert "ssdhip_image_resize_cv_u8" in names and not set(names) & BATCH        # the per-image loop ran


@pytest.mark.gpu
def test_unequal_sizes_without_a_resize_are_refused(monkeypatch):
    """A list without a resize is a copy-kind gather for images that end in one size, NotImplementedError (the loop's case) otherwise."""
    from ssd_keras_amd.data_generator import _image_ops as iop
    n = pc.ns()
    images, _ = pc.mixed_arrays(9, equal=True)
    images[2] = images[2][:-1]
    flipped = lambda: [n.Flip()(iop.ProgramImage.of(*im.shape[:2])) for im in images]
    log = _Launches(monkeypatch)
    with pytest.raises(NotImplementedError):
        iop.run_program_batch(images, flipped())
    assert not log.names                                                 # refused in front of every launch
    images[2] = images[3]
    np.testing.assert_array_equal(iop.run_program_batch(images, flipped()).cpu().numpy(), np.stack([im[:, ::-1] for im in images]))
    assert log.names == ["ssdhip_image_resize_gather_ragged_u8"]
