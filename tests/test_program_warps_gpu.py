"""Lists with Translate / Scale on generate()'s 'program' path (`DataGenerator.compose_warps`) on the GPU: the ragged warp kernel against
the per-image kernel, and composed lists end to end against the per-image loop -- everything bit for bit (the oracle is the existing
per-image code: `iop.warp_affine`, the loop of `generate()`)."""
import numpy as np
import pytest

from tests import program_path_cases as pc
from tests import program_warp_cases as wc

PER_IMAGE = "ssdhip_image_warp_affine_u8"
RAGGED = "ssdhip_image_warp_affine_ragged_u8"
BATCH = {RAGGED, "ssdhip_image_program_ragged_u8", "ssdhip_image_program_ragged_lut_u8", "ssdhip_image_program_hist_u8",
         "ssdhip_image_equalize_tables", "ssdhip_image_resize_gather_ragged_u8", "ssdhip_image_resize_gather_turn_ragged_u8",
         "ssdhip_image_program", "ssdhip_image_program_lut"}
LOOP_NEVER = BATCH - {"ssdhip_image_program", "ssdhip_image_program_lut"}        # the loop's photometric ops launch these two per image
SHAPES = [(1, 1, 3), (5, 3, 3), (7, 9), (8, 6, 4), (40, 32, 3), (16, 8, 3), (37, 53, 3), (61, 45, 3)]
PADDING, BORDER = (9, 200, 3), (255, 0, 77)


class _Launches:
    """The image exports `_native.launch` enqueues, by name."""

    def __init__(self, monkeypatch):
        from ssd_keras_amd import _native as nat
        self.names, real = [], nat.launch

        def logged(name, device, *args):
            if name.startswith("ssdhip_image_"):
                self.names.append(name)
            return real(name, device, *args)
        monkeypatch.setattr(nat, "launch", logged)


def _sources(seed=0):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, size=s).astype(np.uint8) for s in SHAPES]


def _maps(kind, h, w):
    """(ys, xs) over an h x w source."""
    ys, xs = np.arange(h), np.arange(w)
    if kind == "crop":
        return ys[h // 4:max(h // 4 + 1, h - h // 5)], xs[w // 3:max(w // 3 + 1, w - w // 4)]
    if kind == "reversed":
        return ys, xs[::-1]
    if kind == "padded":                                     # a padding on every side and a black row in the middle
        return np.concatenate([[-1], ys[:h // 2], [-2], ys[h // 2:], [-1, -1]]), np.concatenate([[-1, -1], xs, [-1]])
    return ys, xs


def _warps(ha, wa):
    """[(name, M, (out_h, out_w))] for a virtual image of ha x wa."""
    from ssd_keras_amd.data_generator import _image_ops as iop
    centre = (wa / 2, ha / 2)
    out = [("zoom %g" % f, iop.rotation_matrix_2d(centre, 0, f), (ha, wa)) for f in (0.37, 0.5, 1.5, 2.75)]
    shifted = iop.rotation_matrix_2d(centre, 0, 1.3)
    shifted[0, 2] += 2.4
    shifted[1, 2] -= 1.7
    out.append(("zoom and fractional translation", shifted, (ha, wa)))
    out.append(("rotation", iop.rotation_matrix_2d(centre, 30, 0.8), (ha, wa)))
    out.append(("another size", iop.rotation_matrix_2d(centre, 0, 1.2), (max(1, ha - 2), wa + 3)))
    return out


def _staged(iop, ys, xs, M, size, padding=PADDING, border=BORDER):
    return iop.StagedGeoImage(iop.GeoImage(np.asarray(ys), np.asarray(xs), padding), (np.asarray(M, dtype=np.float64), size, border),
                              iop.GeoImage.of(*size))


def _images_of(batch):
    data = batch.data.cpu().numpy()
    return [data[off:off + h * w * c].reshape(h, w, c) for off, h, w, c in batch.table.cpu().numpy()]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["identity", "crop", "reversed", "padded"])
def test_ragged_warp_equals_the_per_image_kernel(kind):
    """Every source shape (one pixel, odd sizes, grey, RGBA, widths that take the dword stores, several workgroups) under every warp
    (image k starts the list at warp k, so one launch mixes them), the A maps of one kind: == `iop.warp_affine` on the image the maps show."""
    from ssd_keras_amd.data_generator import _image_ops as iop
    sources = _sources()
    packed = iop.pack_ragged(sources)
    shown = [wc.from_maps(iop._three_channels(im), *_maps(kind, *im.shape[:2]), PADDING) for im in sources]
    for r in range(7):
        geos, want = [], []
        for k, (im, a) in enumerate(zip(sources, shown)):
            ys, xs = _maps(kind, *im.shape[:2])
            name, M, size = _warps(len(ys), len(xs))[(k + r) % 7]
            geos.append(_staged(iop, ys, xs, M, size))
            want.append((name, iop.warp_affine(np.ascontiguousarray(a), M, (size[1], size[0]), BORDER)))
        batch, after = iop.warp_stage_ragged(packed, geos)
        assert [g.shape for g in after] == [w.shape for _, w in want]
        assert all(int(off) % iop.RAGGED_ALIGN == 0 for off in batch.table.cpu().numpy()[:, 0])
        for k, (got, (name, w)) in enumerate(zip(_images_of(batch), want)):
            np.testing.assert_array_equal(got, w, err_msg="%s maps, image %d %s, %s" % (kind, k, SHAPES[k], name))


@pytest.mark.gpu
@pytest.mark.parametrize("last", [(37, 53, 3), (16, 8, 3), (1, 1, 3)])
def test_source_that_ends_with_its_buffer(last):
    """The last image's final byte is the buffer's: the 8-byte load of its last pixels would end outside, so they are read as bytes."""
    from ssd_keras_amd.data_generator import _image_ops as iop
    rng = np.random.RandomState(5)
    sources = [rng.randint(0, 256, size=(5, 3, 3)).astype(np.uint8), rng.randint(0, 256, size=last).astype(np.uint8)]
    packed = iop.pack_ragged(sources)
    end = int(packed.table[1, 0]) + last[0] * last[1] * 3
    assert end < packed.data.numel()                                        # pack_ragged pads: cut the padding off
    tight = iop.RaggedBatch(packed.data[:end], packed.table, packed.shapes)
    h, w = last[:2]
    for name, M, size in _warps(h, w):
        geos = [_staged(iop, np.arange(5), np.arange(3), np.eye(2, 3), (5, 3)), _staged(iop, np.arange(h), np.arange(w), M, size)]
        batch, _ = iop.warp_stage_ragged(tight, geos)
        got = _images_of(batch)
        np.testing.assert_array_equal(got[0], sources[0])
        np.testing.assert_array_equal(got[1], iop.warp_affine(sources[1], M, (size[1], size[0]), BORDER), err_msg=name)
    # the identity reads the very last pixel with full weight
    batch, _ = iop.warp_stage_ragged(tight, [iop.StagedGeoImage.of(5, 3), iop.StagedGeoImage.of(h, w)])
    np.testing.assert_array_equal(_images_of(batch)[1], sources[1])


@pytest.mark.gpu
def test_an_image_without_a_stage_passes_through_unchanged(monkeypatch):
    """Identity tables and identity maps: byte for byte the image (made 3-channel as the gather reads it), for widths that are and are
    not multiples of 4; its maps stay for the gather."""
    from ssd_keras_amd.data_generator import _image_ops as iop
    sources = _sources(1)
    geos = [iop.StagedGeoImage.of(*im.shape[:2])[::-1].resize(4, 4, iop.INTER_LINEAR) for im in sources]
    log = _Launches(monkeypatch)
    batch, after = iop.warp_stage_ragged(iop.pack_ragged(sources), geos)
    assert log.names == [RAGGED]
    assert [w % 4 for _, w, _ in batch.shapes] == [1, 3, 1, 2, 0, 0, 1, 1]
    for got, im, g, lazy in zip(_images_of(batch), sources, after, geos):
        np.testing.assert_array_equal(got, iop._three_channels(im))
        assert g is lazy.a


def _switched(source, on):
    def make(n):
        g = source(n)
        g.compose_warps = on
        return g
    return make


def _arrays(n):
    return pc.array_generator(n, *pc.mixed_arrays())


def _equal_arrays(n):
    return pc.array_generator(n, *pc.mixed_arrays(8, equal=True))


def _record_stages(monkeypatch):
    """Per batch the program path executes: which of its images carry a stage."""
    from ssd_keras_amd.data_generator import _image_ops as iop
    batches, real = [], iop.run_program_batch

    def run_program_batch(images, lazies):
        batches.append([isinstance(l.geo, iop.StagedGeoImage) and l.geo.stage is not None for l in lazies])
        return real(images, lazies)
    monkeypatch.setattr(iop, "run_program_batch", run_program_batch)
    return batches


def _assert_same(fast, slow):
    assert sorted(fast) == sorted(slow)
    for k in sorted(slow):
        assert fast[k].shape == slow[k].shape and fast[k].dtype == slow[k].dtype, k
        np.testing.assert_array_equal(fast[k], slow[k], err_msg=k)


def _both_routes(monkeypatch, n, source, make_list, seed):
    """(the run with the switch on, its launches, its stages per batch, the per-image loop's run, the loop's launches)."""
    log, stages = _Launches(monkeypatch), _record_stages(monkeypatch)
    fast = pc.run_generate(n, _switched(source, True), make_list(n), seed=seed)
    names = list(log.names)
    monkeypatch.undo()
    log = _Launches(monkeypatch)
    monkeypatch.setattr(n.DataGenerator, "_batch_path", staticmethod(lambda *a: None))
    slow = pc.run_generate(n, _switched(source, False), make_list(n), seed=seed)
    loop_names = list(log.names)
    monkeypatch.undo()
    return fast, names, stages, slow, loop_names


def list_ii_uint8(n):
    """List (ii) with the cast that lets it run at all: RandomBrightness leaves a float64 image (NumPy's uint8 + float), on which the
    per-image loop's own Scale raises TypeError (cv2.warpAffine's stand-in takes uint8) -- the list as first written fails in the loop
    and in the batch alike (`test_a_list_the_loop_refuses_is_refused_alike`).  With ConvertDataType('uint8') behind the brightness it
    is the same shape of list: a first segment, a stage, a translation, the resize, a table step behind it, a float32 batch."""
    ts = wc.list_ii(n)
    return ts[:2] + [n.ConvertDataType('uint8')] + ts[2:]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["i", "ii", "iii", "iv", "v"])
def test_warp_lists_equal_the_per_image_loop(monkeypatch, name):
    """Pixels, dtype, labels, inverters and both generators' final states, two batches of 8, on the fixture dataset and on noise arrays
    (equal sizes for the list without a resize); the launches are the batch's, one ragged warp per batch that has a stage."""
    n = pc.ns()
    make_list = {"i": wc.list_i, "ii": list_ii_uint8, "iii": wc.list_iii, "iv": wc.list_iv, "v": wc.list_v}[name]
    sources = [pc.equal_generator, _equal_arrays] if name == "iii" else [pc.fixture_generator, _arrays]
    staged = mixed = 0
    for k, source in enumerate(sources):
        fast, names, stages, slow, loop_names = _both_routes(monkeypatch, n, source, make_list, seed=50 + k)
        _assert_same(fast, slow)
        assert str(fast["b0_dtype"]) == ("float32" if name == "ii" else "uint8")
        assert len(stages) == 2                                             # both batches were composed
        assert set(names) <= BATCH and PER_IMAGE not in names, names
        assert names.count(RAGGED) == sum(any(b) for b in stages), (names, stages)
        assert not set(loop_names) & LOOP_NEVER, loop_names
        if name == "v":                                                     # the loop's Rotate is a per-image warp launch too
            assert PER_IMAGE in loop_names and "ssdhip_image_resize_gather_turn_ragged_u8" in names
        else:
            assert (PER_IMAGE in loop_names) == any(any(b) for b in stages), loop_names
        staged += sum(sum(b) for b in stages)
        mixed += sum(any(b) and not all(b) for b in stages)
    assert staged >= 1
    if name in ("i", "iv", "v"):
        assert mixed >= 1                                                   # an image without a stage in a batch that has one
    if name in ("ii", "iii"):
        assert all(all(b) for b in stages)


@pytest.mark.gpu
def test_launches_of_list_i(monkeypatch):
    """Switch on: one ragged warp and one gather per batch that has a stage, the gather alone when no image is warped (prob = 0), never
    a per-image launch.  Switch off: the per-image loop, as before."""
    n = pc.ns()
    log, stages = _Launches(monkeypatch), _record_stages(monkeypatch)
    pc.run_generate(n, _switched(_arrays, True), wc.list_i(n), seed=60)
    assert [any(b) for b in stages] == [True, True]
    assert log.names == [RAGGED, "ssdhip_image_resize_gather_ragged_u8"] * 2
    del log.names[:], stages[:]
    pc.run_generate(n, _switched(_arrays, True), wc.list_i(n, prob=0.0), seed=60)
    assert [any(b) for b in stages] == [False, False]
    assert log.names == ["ssdhip_image_resize_gather_ragged_u8"] * 2
    del log.names[:], stages[:]
    pc.run_generate(n, _switched(_arrays, False), wc.list_i(n), seed=60)
    assert not stages and not set(log.names) & LOOP_NEVER and PER_IMAGE in log.names and "ssdhip_image_resize_cv_u8" in log.names


@pytest.mark.gpu
@pytest.mark.parametrize("make_list", [wc.list_two_scales, wc.list_turn_then_scale])
def test_lists_the_lazy_image_refuses_fall_back_to_the_loop(monkeypatch, make_list):
    """Eligible by type, refused when they are recorded: the loop's results, `np.random` and `random` where the loop leaves them."""
    n = pc.ns()
    assert n.DataGenerator._composable(make_list(n), pc.mixed_arrays()[0][2:3], warps=True)
    for source in (pc.fixture_generator, _arrays):
        fast, names, stages, slow, loop_names = _both_routes(monkeypatch, n, source, lambda n: [n.ConvertTo3Channels()] + make_list(n), seed=70)
        _assert_same(fast, slow)
        assert not stages and names == loop_names and PER_IMAGE in names and RAGGED not in names


@pytest.mark.gpu
def test_a_list_the_loop_refuses_is_refused_alike(monkeypatch):
    """List (ii) as first written: Scale on the float64 image a fired RandomBrightness leaves is a TypeError in the per-image loop, so it
    is one under the switch (the batch falls back to the loop from the same draws)."""
    n = pc.ns()

    def outcome(run):
        try:
            return run()
        except TypeError as e:
            return str(e)
    fast = outcome(lambda: pc.run_generate(n, _switched(_arrays, True), wc.list_ii(n), seed=80))
    monkeypatch.setattr(n.DataGenerator, "_batch_path", staticmethod(lambda *a: None))
    slow = outcome(lambda: pc.run_generate(n, _switched(_arrays, False), wc.list_ii(n), seed=80))
    assert isinstance(slow, str) and fast == slow


@pytest.mark.gpu
def test_a_list_without_warps_is_launched_as_before(monkeypatch):
    n = pc.ns()
    runs = []
    for on in (False, True):
        log = _Launches(monkeypatch)
        runs.append((pc.run_generate(n, _switched(pc.fixture_generator, on), pc.list_b(n, (30, 26)), seed=90), list(log.names)))
        monkeypatch.undo()
    _assert_same(runs[1][0], runs[0][0])
    assert runs[1][1] == runs[0][1] and RAGGED not in runs[0][1] and runs[0][1]


@pytest.mark.gpu
def test_a_batch_the_device_decoded_takes_the_program_path_with_warps(monkeypatch, tmp_path):
    """decode = 'device' with `compose_warps`: the route is decided on the device tensors, before they are downloaded for the 'program'
    path, and it is the route of the host-decoded batch -- pixels (the device decoder's are PIL's), labels, inverters and both
    generators' final states are equal, and both runs composed their batch with warps."""
    from PIL import Image
    from ssd_keras_amd.data_generator import jpeg_decode
    from tests import np_jpeg
    n = pc.ns()
    names, labels = [], []
    for k, (h, w) in enumerate([(16, 24), (24, 16), (17, 23), (24, 24)]):
        names.append(str(tmp_path / ("im%d.jpg" % k)))
        Image.fromarray(np_jpeg.make_array(h, w, "RGB", 90 + k)).save(names[-1], quality=85, subsampling=(2, 0, 1, 2)[k])
        labels.append(np.array([[1 + k % 3, 2, 3, w - 3, h - 2]]))
    entered, real = [], n.DataGenerator._transform_batch

    def spy(self, path, transformations, images, labels, want_inverters, warps=False):
        entered.append((path, warps))
        return real(self, path, transformations, images, labels, want_inverters, warps)
    monkeypatch.setattr(n.DataGenerator, "_transform_batch", spy)
    stages = _record_stages(monkeypatch)

    def files(decode):
        def make(n):
            g = n.DataGenerator(filenames=list(names), labels=[l.copy() for l in labels], verbose=False)
            g.decode, g.compose_warps = decode, True
            return g
        return make
    before = dict(jpeg_decode.COUNTERS)
    host = pc.run_generate(n, files('host'), wc.list_i(n), seed=95, n_batches=1, batch_size=4)
    assert jpeg_decode.COUNTERS == before
    dev = pc.run_generate(n, files('device'), wc.list_i(n), seed=95, n_batches=1, batch_size=4)
    assert jpeg_decode.COUNTERS["device"] - before["device"] == 4 and jpeg_decode.COUNTERS["host"] == before["host"]
    _assert_same(dev, host)
    assert entered == [('program', True)] * 2 and len(stages) == 2          # neither run fell back to the loop
