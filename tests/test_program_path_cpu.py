"""generate()'s 'program' path without a GPU: which lists `_batch_path` sends there, and what the lazy `ProgramImage` records."""
import numpy as np
import pytest

from tests import program_path_cases as pc


def _rgb(*sizes):
    return [np.zeros((h, w, 3), dtype=np.uint8) for h, w in sizes]


def _mixed():
    return [np.zeros((7, 9), dtype=np.uint8), np.zeros((8, 6, 4), dtype=np.uint8), np.zeros((5, 3, 3), dtype=np.uint8)]


@pytest.mark.parametrize("name", sorted(pc.LISTS))
def test_accepted_lists_take_the_program_path(name):
    n = pc.ns()
    images = _rgb((18, 22), (18, 22)) if name == "e" else _mixed()
    for have_labels in (True, False):
        assert n.DataGenerator._batch_path(pc.LISTS[name](n), images, have_labels) == 'program'


def test_more_accepted_lists():
    n = pc.ns()
    path = lambda ts, images=None: n.DataGenerator._batch_path(ts, images or _rgb((7, 9), (8, 6)), True)
    gen = n.PatchCoordinateGenerator(must_match='w_ar', min_scale=0.3, max_scale=1.0, scale_uniformly=False, min_aspect_ratio=0.5,
                                     max_aspect_ratio=2.0)
    assert path([n.RandomGamma(), n.Resize(8, 8)]) == 'program'
    assert path([n.Brightness(3), n.Hue(4), n.Flip('vertical'), n.Crop(1, 1, 1, 1), n.Pad(1, 2, 3, 4), n.ResizeRandomInterp(8, 8)]) == 'program'
    assert path([n.RandomPatch(gen), n.RandomPatchInf(gen), n.RandomMaxCropFixedAR(1.0), n.CropPad(0, 0, 4, 4), n.Rotate(90),
                 n.Resize(8, 8), n.ChannelSwap((2, 1, 0)), n.Gamma(2.0)]) == 'program'
    assert path([n.ConvertTo3Channels(), n.Contrast(1.2), n.Saturation(1.1), n.HistogramEqualization()], _mixed()) == 'program'
    assert path([n.ConvertTo3Channels(), n.Resize(8, 8), n.RandomSaturation()], _mixed()) == 'program'      # Resize returns a fresh array


def test_old_lists_keep_their_paths():
    n = pc.ns()
    path = n.DataGenerator._batch_path
    mixed, equal = _mixed(), _rgb((18, 22), (18, 22))
    assert path([n.ConvertTo3Channels(), n.Resize(300, 300)], mixed, False) == 'gather'
    assert path([n.ConvertTo3Channels(), n.RandomPadFixedAR(1.0), n.Resize(300, 300)], mixed, True) == 'gather'
    assert path([n.SSDDataAugmentation(300, 300)], mixed, True) == 'ssd'
    assert path([n.DataAugmentationConstantInputSize()], equal, True) == 'constant'
    assert path([n.DataAugmentationVariableInputSize(300, 300)], mixed, True) == 'variable'
    assert path([n.DataAugmentationSatellite(300, 300)], mixed, True) == 'satellite'
    # what was the per-image loop for them stays the loop
    assert path([n.SSDDataAugmentation(300, 300)], mixed, False) is None
    assert path([n.DataAugmentationConstantInputSize()], _rgb((18, 22), (18, 23)), True) is None


def _rejected(n):
    class MyResize(n.Resize):
        pass
    rotate = n.Rotate(90)
    rotate.angle = 45
    random_rotate = n.RandomRotate([90])
    random_rotate.angles = [90, 30]
    rgb = None
    return {
        "translate": ([n.Translate(0.1, 0.1), n.Resize(8, 8)], rgb),
        "scale": ([n.RandomScale(), n.Resize(8, 8)], rgb),
        "callable": ([n.Brightness(3), lambda image, labels=None: image], rgb),
        "subclass": ([MyResize(8, 8)], rgb),
        "chain inside a longer list": ([n.SSDDataAugmentation(8, 8), n.Brightness(3)], rgb),
        "photometric chain object": ([n.SSDPhotometricDistortions(), n.Resize(8, 8)] if hasattr(n, "SSDPhotometricDistortions")
                                     else [n.SSDDataAugmentation(8, 8).photometric_distortions, n.Resize(8, 8)], rgb),
        "free-angle rotate": ([rotate, n.Resize(8, 8)], rgb),
        "free-angle random rotate": ([random_rotate, n.Resize(8, 8)], rgb),
        "geometry behind the second segment": ([n.Resize(8, 8), n.Brightness(3), n.Flip()], rgb),
        "two resizes": ([n.Resize(8, 8), n.Resize(4, 4)], rgb),
        "resize not the last geometric op": ([n.Resize(8, 8), n.Flip()], rgb),
        "keep_3ch=False": ([n.ConvertColor(current='RGB', to='GRAY', keep_3ch=False), n.Resize(8, 8)], rgb),
        "channels": ([n.Brightness(3), n.ConvertTo3Channels(), n.Resize(8, 8)], _mixed()),
        "in-place op first": ([n.ConvertTo3Channels(), n.RandomHue(), n.Resize(8, 8)], rgb),
        "in-place op behind a view": ([n.Flip(), n.Crop(1, 1, 1, 1), n.HistogramEqualization()], rgb),
        "in-place op behind a conditional copy": ([n.RandomBrightness(), n.Saturation(1.5), n.Resize(8, 8)], rgb),
    }


@pytest.mark.parametrize("rule", ["translate", "scale", "callable", "subclass", "chain inside a longer list", "photometric chain object",
                                  "free-angle rotate", "free-angle random rotate", "geometry behind the second segment", "two resizes",
                                  "resize not the last geometric op", "keep_3ch=False", "channels", "in-place op first",
                                  "in-place op behind a view", "in-place op behind a conditional copy"])
def test_rejected_lists_stay_in_the_loop(rule):
    n = pc.ns()
    transformations, images = _rejected(n)[rule]
    assert n.DataGenerator._batch_path(transformations, images or _rgb((7, 9), (8, 6)), True) is None


def test_images_that_are_not_uint8_arrays_stay_in_the_loop():
    n = pc.ns()
    assert n.DataGenerator._batch_path(pc.list_c(n), [np.zeros((4, 4, 3), dtype=np.float32)], True) is None


def _walk(n, transformations, image):
    for t in transformations:
        image = t(image)
    return image


def test_fixed_lists_record_their_steps():
    from ssd_keras_amd.data_generator import _image_ops as iop
    n = pc.ns()
    gamma = n.Gamma(2.0)
    ts = [n.ConvertTo3Channels(), n.ConvertDataType('float32'), n.Brightness(10), n.Contrast(1.5), n.ConvertDataType('uint8'),
          n.ConvertColor(current='RGB', to='HSV'), n.Saturation(1.25), n.Hue(7), n.HistogramEqualization(),
          n.ConvertColor(current='HSV', to='RGB'), gamma, n.ChannelSwap((2, 0, 1)), n.Flip(), n.Resize(8, 6), n.Brightness(-3)]
    image, dtypes = iop.ProgramImage.of(5, 7), []
    for t in ts:
        image = t(image)
        dtypes.append(str(image.dtype))
    assert dtypes == ['uint8', 'float32', 'float32', 'float32', 'uint8', 'uint8', 'uint8', 'uint8', 'uint8', 'uint8', 'uint8', 'uint8',
                      'uint8', 'uint8', 'float64']
    assert [s[0] for s in image.pre] == ['to_f32', 'brightness', 'contrast', 'to_u8', 'rgb2hsv', 'saturation', 'hue', 'equalize', 'hsv2rgb',
                                         'gamma', 'swap']
    assert image.pre[:7] == [('to_f32', 0), ('brightness', 10), ('contrast', 1.5), ('to_u8', 0), ('rgb2hsv', 0), ('saturation', 1.25),
                             ('hue', 7)]
    assert image.pre[7] == ('equalize', 2) and image.pre[8] == ('hsv2rgb', 0) and image.pre[10] == ('swap', 2 + 4 * 0 + 16 * 1)
    np.testing.assert_array_equal(image.pre[9][1], gamma.table)
    assert image.post == [('brightness', -3)]
    assert image.shape == (8, 6, 3) and image.ndim == 3
    assert image.geo.resized == (8, 6, 1) and list(image.geo.xs) == [6, 5, 4, 3, 2, 1, 0] and list(image.geo.ys) == [0, 1, 2, 3, 4]
    # the same ops on a NumPy image see the same dtypes
    assert str(iop.end_dtype(np.uint8, [s for s in image.pre if s[0] not in ('gamma', 'equalize')] + image.post)) == 'float64'


def test_labels_and_inverters_pass_through():
    from ssd_keras_amd.data_generator import _image_ops as iop
    n = pc.ns()
    labels = np.array([[1, 2, 1, 5, 4]])
    image, out = n.Hue(4)(iop.ProgramImage.of(5, 7), labels)
    assert out is labels and image.pre == [('hue', 4)]
    image, out, inverter = n.Resize(10, 14)(image, labels, return_inverter=True)
    np.testing.assert_array_equal(out, [[1, 4, 2, 10, 8]])
    assert image.shape == (10, 14, 3) and callable(inverter)


def test_what_numpy_refuses_is_refused_when_recorded():
    from ssd_keras_amd.data_generator import _image_ops as iop
    n = pc.ns()
    f32 = n.ConvertDataType('float32')(iop.ProgramImage.of(5, 7))
    f64 = n.Brightness(3)(iop.ProgramImage.of(5, 7))
    host32, host64 = np.zeros((5, 7, 3), dtype=np.float32), np.zeros((5, 7, 3), dtype=np.float64)
    for lazy, host, op in ((f32, host32, n.HistogramEqualization()), (f32, host32, n.Gamma(2.0)), (f64, host64, n.Gamma(2.0)),
                           (f64, host64, n.ConvertColor(current='RGB', to='HSV')), (f64, host64, n.ConvertColor(current='RGB', to='GRAY'))):
        with pytest.raises(TypeError) as recorded:
            op(lazy)
        with pytest.raises(TypeError) as direct:                         # raised in front of any launch
            op(host)
        assert str(recorded.value) == str(direct.value)


def test_what_cannot_be_composed_raises_not_implemented():
    from ssd_keras_amd.data_generator import _image_ops as iop
    n = pc.ns()
    second = n.Brightness(3)(n.Resize(8, 6)(n.ConvertDataType('uint8')(iop.ProgramImage.of(5, 7))))
    assert second.post == [('brightness', 3)] and second.pre == [('to_u8', 0)]
    for op in (n.Flip(), n.Resize(4, 4), n.Crop(1, 1, 1, 1), n.Rotate(90)):
        with pytest.raises(NotImplementedError):
            op(n.ConvertDataType('uint8')(second))                      # uint8 again, but behind a second-segment step
    with pytest.raises(NotImplementedError):
        n.Flip()(n.ConvertDataType('float32')(iop.ProgramImage.of(5, 7)))          # geometry on a float state
    fifteen = _walk(n, [n.ChannelSwap((1, 0, 2))] * 15, iop.ProgramImage.of(5, 7))
    assert len(fifteen.pre) == 15
    with pytest.raises(NotImplementedError):
        n.ChannelSwap((1, 0, 2))(fifteen)                               # the 16th step of a segment
    assert len(n.ChannelSwap((1, 0, 2))(n.Flip()(fifteen)).post) == 1   # the second segment counts for itself
    four = _walk(n, [n.Gamma(2.0), n.HistogramEqualization(), n.Gamma(0.5), n.HistogramEqualization()], iop.ProgramImage.of(5, 7))
    for op in (n.Gamma(1.5), n.HistogramEqualization()):
        with pytest.raises(NotImplementedError):
            op(four)                                                    # a fifth table
    with pytest.raises(NotImplementedError):
        n.ConvertColor(current='RGB', to='GRAY', keep_3ch=False)(iop.ProgramImage.of(5, 7))


def test_segment_tables_deal_slots_in_step_order():
    from ssd_keras_amd.data_generator import _image_ops as iop
    table = np.arange(256, dtype=np.uint8)[::-1]
    programs = [[('rgb2hsv', 0), ('equalize', 2), ('hsv2rgb', 0), ('gamma', table), ('equalize', 0)], [], [('gamma', table)]]
    plain, luts, equalizes, used = iop._segment_tables(programs)
    assert used and plain[0] == [('rgb2hsv', 0), ('lut', 0 + 4 * 4), ('hsv2rgb', 0), ('lut', 1 + 4 * 7), ('lut', 2 + 4 * 1)]
    assert plain[1] == [] and plain[2] == [('lut', 0 + 4 * 7)]
    assert equalizes == [[(1, 2, 0), (4, 0, 2)], [], []]
    np.testing.assert_array_equal(luts[0, 1], table)
    np.testing.assert_array_equal(luts[2, 0], table)
    assert not luts[1].any() and not luts[0, 0].any()
    assert iop._segment_tables([[('hue', 3)]])[3] is False


def test_program_check_is_a_host_function():
    """ssdhip_image_program_check needs no device: op 11 is refused without tables, on a float state, and with a malformed argument."""
    from ssd_keras_amd import _native as nat
    from ssd_keras_amd.data_generator import _image_ops as iop

    def check(steps, in_code=nat.IMG_U8, have_luts=True):
        ops, args = iop.encode(steps)
        nat.image_program_check(ops[None], args[None], in_code, have_luts)
    check([('rgb2hsv', 0), ('lut', 3 + 4 * 7), ('to_f32', 0)])
    check([('to_u8', 0), ('lut', 4)], in_code=nat.IMG_F32)
    for steps, kw in (([('lut', 4)], dict(have_luts=False)), ([('to_f32', 0), ('lut', 4)], {}), ([('brightness', 1), ('lut', 4)], {}),
                      ([('lut', 4)], dict(in_code=nat.IMG_F64)), ([('lut', 3)], {}), ([('lut', 32)], {}), ([('lut', 4.5)], {})):
        with pytest.raises(nat.SsdHipError):
            check(steps, **kw)
    ops, args = iop.encode([('hue', 1)])
    ops[1] = 12
    with pytest.raises(nat.SsdHipError):
        nat.image_program_check(ops[None], args[None], nat.IMG_U8, True)
