"""NumPy restatement of const_plan_kernel (csrc/ssdhip_augment.hip): the geometry rows the constant-input-size chain's decision kernel
writes -> what ssdhip_image_warp_affine_u8 takes, operation by operation as the kernel does them in float64.  The CPU tests hold it
against `_image_ops.WarpImage.plan()`, the GPU tests hold the kernel against both."""
import numpy as np

GEO = 8          # sequence, translated?, dx, dy, scaled?, factor, flipped?, zoom first?


def row(seq=1, shift=None, factor=None, flip=False):
    """One geometry row: `shift` = (dx, dy) whole pixels or None, `factor` the zoom or None; sequence 2 zooms before it translates."""
    g = np.zeros(GEO, dtype=np.float64)
    g[0], g[5], g[7] = seq, 1.0, float(seq == 2)
    if shift is not None:
        g[1], g[2], g[3] = 1.0, shift[0], shift[1]
    if factor is not None:
        g[4], g[5] = 1.0, factor
    g[6] = float(flip)
    return g


def matrix(factor, H, W):
    """cv2.getRotationMatrix2D((W / 2, H / 2), 0, factor): the centre rounded to float32, then float64."""
    f = np.float64
    cx, cy = f(np.float32(f(W) / f(2.0))), f(np.float32(f(H) / f(2.0)))
    a, b = f(1.0) * f(factor), f(0.0) * f(factor)
    return [a, b, (f(1.0) - a) * cx - b * cy, -b, a, b * cx + (f(1.0) - a) * cy]


def plans(geometry, H, W):
    """geometry (B, 8) float64 -> (geo (B, 5) int32, xtab (B, W, 2) int32, ytab (B, H, 2) int32)."""
    geometry = np.asarray(geometry, dtype=np.float64).reshape(-1, GEO)
    B = geometry.shape[0]
    geo = np.zeros((B, 5), dtype=np.int32)
    xtab = np.zeros((B, W, 2), dtype=np.int32)
    ytab = np.zeros((B, H, 2), dtype=np.int32)
    f = np.float64
    for b, g in enumerate(geometry):
        translated, scaled = g[1] != 0.0, (g[4] != 0.0 and g[5] != 1.0)
        post = translated and scaled and g[7] != 0.0
        dx, dy = (int(g[2]), int(g[3])) if translated else (0, 0)
        geo[b] = (int(g[6] != 0.0), 0 if post else dx, 0 if post else dy, dx if post else 0, dy if post else 0)
        m = matrix(g[5], H, W) if scaled else [f(1.0), f(0.0), f(0.0), f(0.0), f(1.0), f(0.0)]
        d = m[0] * m[4] - m[1] * m[3]
        d = f(1.0) / d if d != 0.0 else f(0.0)
        a11, a22 = m[4] * d, m[0] * d
        m[0], m[1], m[3], m[4] = a11, m[1] * -d, m[3] * -d, a22
        b1 = -m[0] * m[2] - m[1] * m[5]
        b2 = -m[3] * m[2] - m[4] * m[5]
        m[2], m[5] = b1, b2
        x, y = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
        xtab[b, :, 0] = np.rint(m[0] * x * 1024.0).astype(np.int32)
        xtab[b, :, 1] = np.rint(m[3] * x * 1024.0).astype(np.int32)
        ytab[b, :, 0] = (np.rint((m[1] * y + m[2]) * 1024.0) + 16.0).astype(np.int32)
        ytab[b, :, 1] = (np.rint((m[4] * y + m[5]) * 1024.0) + 16.0).astype(np.int32)
    return geo, xtab, ytab


def hand_cases():
    """[(name, geometry row, the WarpImage the chain's ops record for it)] for an image of any size: translation only, zoom only,
    translate then zoom in (sequence 1), zoom out then translate (sequence 2), each with and without the flip."""
    cases = []
    for flip in (False, True):
        tag = " + flip" if flip else ""
        cases += [("translation only" + tag, row(1, shift=(-7, 5), flip=flip), dict(seq=1, shift=(-7, 5), factor=None, flip=flip)),
                  ("translation only, sequence 2" + tag, row(2, shift=(9, -4), flip=flip), dict(seq=2, shift=(9, -4), factor=None, flip=flip)),
                  ("zoom in only" + tag, row(1, factor=1.3724, flip=flip), dict(seq=1, shift=None, factor=1.3724, flip=flip)),
                  ("zoom out only" + tag, row(2, factor=0.6181, flip=flip), dict(seq=2, shift=None, factor=0.6181, flip=flip)),
                  ("translate then zoom in" + tag, row(1, shift=(11, -3), factor=1.9021, flip=flip),
                   dict(seq=1, shift=(11, -3), factor=1.9021, flip=flip)),
                  ("zoom out then translate" + tag, row(2, shift=(-6, 13), factor=0.5013, flip=flip),
                   dict(seq=2, shift=(-6, 13), factor=0.5013, flip=flip)),
                  ("nothing" + tag, row(1, flip=flip), dict(seq=1, shift=None, factor=None, flip=flip))]
    return cases


def warp_image_of(case, H, W, background=(0, 0, 0)):
    """The lazy image Translate / Scale / Flip record for a hand case, through the ops' own calls to `_image_ops.warp_affine`."""
    from ssd_keras_amd.data_generator import _image_ops as iop
    img = iop.WarpImage.of(H, W)

    def translate(img):
        if case["shift"] is None:
            return img
        dx, dy = case["shift"]
        return iop.warp_affine(img, np.float32([[1, 0, dx], [0, 1, dy]]), (W, H), background)

    def zoom(img):
        if case["factor"] is None:
            return img
        return iop.warp_affine(img, iop.rotation_matrix_2d((W / 2, H / 2), 0, case["factor"]), (W, H), background)

    img = zoom(translate(img)) if case["seq"] == 1 else translate(zoom(img))
    return img[:, ::-1] if case["flip"] else img
