"""Transformation lists with Translate / Scale for generate()'s 'program' path under `compose_warps` (tests/test_program_warps_cpu.py,
tests/test_program_warps_gpu.py, tools/time_program_path.py), and the NumPy statement of what a recorded `StagedGeoImage` means: the A
maps, cv2.warpAffine (tests/np_warp.py), the B maps with cv2.resize (oracle/np_image.py)."""
import numpy as np

from tests import np_warp


def list_i(n, size=(30, 26), prob=0.5):
    """DataAugmentationConstantInputSize's geometry for images of mixed sizes."""
    return [n.ConvertTo3Channels(), n.RandomTranslate(prob=prob), n.RandomScale(prob=prob), n.RandomFlip(), n.Resize(size[0], size[1])]


def list_ii(n, size=(25, 27)):
    """Both photometric segments around a fixed zoom and a fixed translation; a float32 batch out."""
    return [n.ConvertTo3Channels(), n.RandomBrightness(), n.Scale(0.7), n.Translate(0.1, -0.2), n.Resize(size[0], size[1]), n.RandomGamma(),
            n.ConvertDataType('float32')]


def list_iii(n):
    """No resize: images of one size only."""
    return [n.RandomScale(prob=1.0), n.RandomFlip()]


def list_iv(n, size=(30, 26)):
    """A random patch in front of a zoom that validates its boxes."""
    validator = n.ImageValidator(overlap_criterion='area', bounds=(0.3, 1.0), n_boxes_min=1)
    box_filter = n.BoxFilter(check_overlap=True, check_min_area=True, check_degenerate=True, overlap_criterion='area',
                             overlap_bounds=(0.3, 1.0), min_area=4)
    return [n.ConvertTo3Channels(),
            n.RandomPatch(n.PatchCoordinateGenerator(must_match='h_w', min_scale=0.5, max_scale=1.5, scale_uniformly=False), prob=0.7,
                          background=(7, 8, 9)),
            n.RandomScale(prob=0.5, image_validator=validator, box_filter=box_filter, background=(90, 1, 200)),
            n.Resize(size[0], size[1])]


def list_v(n, size=(26, 30)):
    """A quarter turn BEHIND the zoom: a turn of the B maps for an image with a stage, of its own maps (transposed) for one without."""
    return [n.ConvertTo3Channels(), n.RandomScale(prob=0.5, background=(0, 120, 255)), n.RandomRotate(angles=[90, 180, 270], prob=0.7),
            n.Resize(size[0], size[1])]


def list_translate(n, size=(30, 26)):
    return [n.Translate(0.2, -0.1), n.Resize(size[0], size[1])]


def list_scale(n, size=(30, 26)):
    return [n.RandomScale(), n.Resize(size[0], size[1])]


def list_two_scales(n, size=(30, 26)):
    """Two non-integer warps: eligible by type, refused when it is recorded."""
    return [n.Scale(0.5), n.Scale(1.5), n.Resize(size[0], size[1])]


def list_turn_then_scale(n, size=(30, 26)):
    """A quarter turn in front of a warp: eligible by type, refused when it is recorded."""
    return [n.Rotate(90), n.Scale(0.5), n.Resize(size[0], size[1])]


def from_maps(image, ys, xs, padding):
    """The virtual image two index maps show of a 3-channel image: -1 = the padding colour, -2 = black."""
    ys, xs = np.asarray(ys), np.asarray(xs)
    out = image[np.clip(ys, 0, None)][:, np.clip(xs, 0, None)].copy()
    pad = np.array(padding if padding is not None else (0, 0, 0), dtype=np.uint8)
    out[ys == -1, :] = pad
    out[:, xs == -1] = pad
    out[ys == -2, :] = 0
    out[:, xs == -2] = 0
    return out


def _from_geo(image, geo):
    from oracle import np_image as npi
    if geo.transposed:
        image = image.transpose(1, 0, 2)
    out = from_maps(image, geo.ys, geo.xs, geo.background)
    if geo.resized is not None:
        out = npi.resize(np.ascontiguousarray(out), (geo.resized[1], geo.resized[0]), geo.resized[2])
    return out


def materialise(image, staged):
    """A recorded `StagedGeoImage` over a 3-channel image, executed in NumPy."""
    if staged.stage is None:
        return _from_geo(image, staged.a)
    M, (out_h, out_w), border = staged.stage
    warped = np_warp.warp_affine(np.ascontiguousarray(_from_geo(image, staged.a)), M, (out_w, out_h), border)
    return _from_geo(warped, staged.b)


def install_numpy_kernels(monkeypatch):
    """The ops' eager path on NumPy images without a GPU: cv2.warpAffine by tests/np_warp.py, cv2.resize by oracle/np_image.py."""
    from oracle import np_image as npi
    from ssd_keras_amd.data_generator import _image_ops as iop
    real_warp, real_resize = iop.warp_affine, iop.resize

    def warp_affine(image, M, dsize, background=0):
        if isinstance(image, np.ndarray):
            return np_warp.warp_affine(np.ascontiguousarray(image), M, (int(dsize[0]), int(dsize[1])), background)
        return real_warp(image, M, dsize, background)

    def resize(image, out_h, out_w, interp):
        if isinstance(image, np.ndarray):
            return npi.resize(np.ascontiguousarray(image), (out_w, out_h), interp)
        return real_resize(image, out_h, out_w, interp)

    monkeypatch.setattr(iop, "warp_affine", warp_affine)
    monkeypatch.setattr(iop, "resize", resize)
