"""Host side of the device JPEG decoder, without a GPU: the NumPy restatement (tests/np_jpeg.py) against PIL on the whole grid, and
`jpeg_decode.plan_jpeg` -- what it accepts, what it refuses, and that no cut of a file makes it raise or point outside the file."""
import io

import numpy as np
import pytest

from tests import np_jpeg


@pytest.fixture(scope="module")
def grid():
    return np_jpeg.grid()


def test_restatement_equals_pil_on_the_grid(grid):
    assert len(grid) == 448
    for key, data in grid:
        want = np_jpeg.pil_decode(data)
        got, status = np_jpeg.decode(data)
        assert status == 0, key
        assert got.dtype == want.dtype == np.uint8 and got.shape == want.shape, key
        assert np.array_equal(got, want), key


@pytest.mark.parametrize("size", [(2, 3), (5, 4), (9, 5), (7, 6)])
def test_restatement_at_downsampled_widths_up_to_two(size):
    """libjpeg replicates a chroma plane of at most two columns and filters a wider one: both sides of that threshold."""
    for sub in (1, 2):
        data = np_jpeg.make_jpeg(size[0], size[1], sub, 90, seed=size[1])
        got, status = np_jpeg.decode(data)
        assert status == 0 and np.array_equal(got, np_jpeg.pil_decode(data)), (size, sub)


def test_restart_markers_are_in_the_grid(grid):
    """The grid's restart_marker_blocks=2 members really carry a restart interval (PIL honours the keyword)."""
    with_restart = [np_jpeg.parse(data) for key, data in grid if key[5] == 2]
    assert all(p.interval == 2 for p in with_restart)
    assert any(len(p.segments) > 1 for p in with_restart)


def test_plan_refuses_what_the_kernels_do_not_decode():
    from PIL import Image
    from ssd_keras_amd.data_generator.jpeg_decode import plan_jpeg
    rgb = Image.fromarray(np_jpeg.make_array(24, 40, "RGB", 1))
    buf = io.BytesIO()
    rgb.save(buf, "JPEG", progressive=True)
    assert plan_jpeg(buf.getvalue()) is None
    buf = io.BytesIO()
    rgb.convert("CMYK").save(buf, "JPEG")
    assert plan_jpeg(buf.getvalue()) is None
    buf = io.BytesIO()
    rgb.save(buf, "PNG")
    assert plan_jpeg(buf.getvalue()) is None
    assert plan_jpeg(b"") is None and plan_jpeg(b"\xff\xd8\xff") is None
    buf = io.BytesIO()
    rgb.save(buf, "JPEG", subsampling=0, keep_rgb=True)          # Adobe transform 0: components are R, G, B
    assert plan_jpeg(buf.getvalue()) is None


def test_plan_geometry_tables_and_restart_ranges(grid):
    from ssd_keras_amd.data_generator.jpeg_decode import plan_jpeg
    for key, data in grid[::3]:
        h, w, sub, q, opt, rst = key
        plan, ref = plan_jpeg(data), np_jpeg.parse(data)
        assert plan is not None, key
        hs, vs, mcux, mcuy, _ = np_jpeg.geometry(ref)
        assert (plan.height, plan.width, plan.ncomp) == (h, w, 1 if sub == "L" else 3), key
        assert (plan.hs, plan.vs) == (hs, vs) == {0: (1, 1), 1: (2, 1), 2: (2, 2), "L": (1, 1)}[sub], key
        assert (plan.mcux, plan.mcuy) == (mcux, mcuy), key
        assert plan.shape == np_jpeg.pil_decode(data).shape, key
        assert plan.qt_ids == [c[3] for c in ref.comps], key
        assert plan.dc_ids == [s[0] for s in ref.scan] and plan.ac_ids == [s[1] for s in ref.scan], key
        for c in range(plan.ncomp):
            assert np.array_equal(plan.qtables[c], ref.qt[ref.comps[c][3]]), key
            assert (list(plan.dc_tables[c][0]), list(plan.dc_tables[c][1])) == (ref.huff[(0, ref.scan[c][0])]), key
            assert (list(plan.ac_tables[c][0]), list(plan.ac_tables[c][1])) == (ref.huff[(1, ref.scan[c][1])]), key
        assert plan.restart_interval == rst == ref.interval, key
        assert plan.segments == ref.segments, key
        assert len(plan.segments) == (-(-mcux * mcuy // rst) if rst else 1), key
        assert plan.has_eoi and data[plan.segments[-1][1]:plan.segments[-1][1] + 2] == b"\xff\xd9", key
        for b, e in plan.segments[:-1]:
            assert data[e] == 0xFF and 0xD0 <= data[e + 1] <= 0xD7, key


def test_plan_of_a_file_cut_anywhere(grid):
    """A file cut off at every one of its first 700 byte positions: None, or a plan whose every range lies inside the bytes."""
    from ssd_keras_amd.data_generator.jpeg_decode import plan_jpeg
    picks = [d for k, d in grid if k[:2] == (33, 50) and k[3] == 95 and not k[4]]
    assert len(picks) == 8
    planned = 0
    for data in picks:
        for cut in range(min(700, len(data))):
            part = data[:cut]
            plan = plan_jpeg(part)
            if plan is None:
                continue
            planned += 1
            assert not plan.has_eoi
            assert all(0 <= b <= e <= len(part) for b, e in plan.segments)
    assert planned > 0                                           # cuts inside the scan keep a plan: the device reports those


def test_decode_switch_of_the_generator():
    from ssd_keras_amd.data_generator.object_detection_2d_data_generator import DataGenerator
    """'host' is the default, 'device' the opt-in, anything else is refused -- through the attribute and through `with_decode`; the
    constructor keeps the reference's parameters (test_data_generator_cpu.py pins them)."""
    assert DataGenerator().decode == "host"
    assert DataGenerator.with_decode("host").decode == "host"
    assert DataGenerator.with_decode("device", verbose=False).decode == "device"
    g = DataGenerator()
    g.decode = "device"
    assert g.decode == "device" and DataGenerator().decode == "host"
    for bad in ("gpu", None, True, "Device"):
        with pytest.raises(ValueError):
            DataGenerator.with_decode(bad)
        with pytest.raises(ValueError):
            g.decode = bad
    assert g.decode == "device"
    with pytest.raises(TypeError):
        DataGenerator(decode="device")
