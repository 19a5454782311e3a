"""Host side of the image half of the augmentation: per-image programs for `ssdhip_image_program`, tap tables for
`ssdhip_image_resize_cv_u8` (cv2.resize's own 8-bit arithmetic), histogram equalisation and look-up tables -- the pixel work itself runs in csrc/ssdhip_image.hip.
Images come in as the reference's ops take them (one NumPy array (H, W, 3), uint8 or float32) or as a CUDA tensor (B, H, W, 3);
NumPy in -> NumPy out (one upload, one download), tensor in -> tensor out (nothing crosses PCIe)."""
from __future__ import annotations

import numpy as np

from .. import _native as nat

U8, F32, F64 = "uint8", "float32", "float64"
_NP = {U8: np.uint8, F32: np.float32, F64: np.float64}


def end_dtype(dtype, steps):
    """The dtype a program ends in, following NumPy's rules for the reference's expressions (see csrc/ssdhip_image.hip)."""
    tag = str(np.dtype(dtype))
    if tag not in _NP:
        raise TypeError("images are uint8, float32 or float64 arrays, not %s" % tag)
    for name, _ in steps:
        if name == "to_f32":
            tag = F32
        elif name == "to_u8":
            tag = U8
        elif name in ("brightness", "contrast"):
            tag = F32 if tag == F32 else F64
        elif name in ("rgb2hsv", "hsv2rgb", "rgb2gray") and tag == F64:
            raise TypeError("colour conversions take uint8 or float32 images (cv2.cvtColor does not take float64)")
    return tag


def encode(steps):
    """[(name, argument), ...] -> (ops int32[16], args float64[16])."""
    if len(steps) > nat.IMG_PROG - 1:
        raise ValueError("a program holds at most %d steps" % (nat.IMG_PROG - 1))
    ops = np.zeros(nat.IMG_PROG, dtype=np.int32)
    args = np.zeros(nat.IMG_PROG, dtype=np.float64)
    for k, (name, arg) in enumerate(steps):
        ops[k] = nat.IMG_OPS[name]
        args[k] = float(arg)
    return ops, args


def swap_code(order):
    o = tuple(int(v) for v in order)
    if len(o) != 3 or any(v not in (0, 1, 2) for v in o):
        raise ValueError("a channel order is three indices out of (0, 1, 2)")
    return o[0] + 4 * o[1] + 16 * o[2]


def _torch_dtype(tag):
    import torch
    return {U8: torch.uint8, F32: torch.float32, F64: torch.float64}[tag]


def run(image, steps):
    """One program on one image (NumPy (H, W, 3)) or the same program on every image of a CUDA batch (B, H, W, 3); a lazy `ProgramImage`
    records the steps instead."""
    import torch
    if isinstance(image, ProgramImage):
        return image.record(steps)
    if isinstance(image, np.ndarray):
        if image.ndim != 3 or image.shape[2] != 3:
            raise ValueError("expected an (H, W, 3) image")
        out_tag = end_dtype(image.dtype, steps)
        ops, args = encode(steps)
        dev = nat.to_device(np.ascontiguousarray(image)[None])
        out = nat.image_program(dev, ops[None], args[None], _torch_dtype(out_tag))
        return out[0].cpu().numpy()
    out_tag = end_dtype(str(image.dtype).replace("torch.", ""), steps)
    ops, args = encode(steps)
    b = image.shape[0]
    return nat.image_program(image.contiguous(), np.repeat(ops[None], b, 0), np.repeat(args[None], b, 0), _torch_dtype(out_tag))


def run_batch(images, programs):
    """Per-image programs on a CUDA uint8 / float32 batch (B, H, W, 3): `programs[i]` is image i's step list; all must end in one dtype."""
    tags = {end_dtype(str(images.dtype).replace("torch.", ""), p) for p in programs}
    if len(tags) != 1:
        raise ValueError("the programs of a batch must end in the same dtype")
    enc = [encode(p) for p in programs]
    return nat.image_program(images.contiguous(), np.stack([e[0] for e in enc]), np.stack([e[1] for e in enc]), _torch_dtype(tags.pop()))


# ---- lazy geometry: the geometric ops of a chain recorded instead of executed ----------------------------------------------------------
class GeoImage:
    """An image that EXISTS ONLY AS INDEX MAPS into an image resident on the device: what the geometric ops of the augmentation chain
    (expansion / crop = a window with a background, flips = reversed slices, rotations by quarter turns, the final resize) do to it is
    recorded as two index arrays -- `ys[i]` / `xs[j]` = the row / column of the original image that row i / column j of the current
    virtual image shows, -1 = a position filled with `background`, -2 = a position a rotation left black -- and executed once, for a
    whole batch, by `ssdhip_image_resize_gather_cv_u8` (its `_turn` form when an image has rotated).  `transposed`: after a rotation
    by 90 or 270 degrees `ys` addresses the original's COLUMNS and `xs` its rows.  Quacks like the (H, W, 3) uint8 array the ops expect:
    `shape`, `ndim`, `dtype`, slicing with plain / reversed slices."""

    ndim = 3
    dtype = np.dtype(np.uint8)

    def __init__(self, ys, xs, background=None, resized=None, transposed=False):
        self.ys, self.xs, self.background, self.resized, self.transposed = ys, xs, background, resized, bool(transposed)

    @classmethod
    def of(cls, height, width):
        return cls(np.arange(height, dtype=np.int64), np.arange(width, dtype=np.int64))

    @property
    def shape(self):
        if self.resized is not None:
            return (self.resized[0], self.resized[1], 3)
        return (len(self.ys), len(self.xs), 3)

    @property
    def turned(self):
        """Whether a rotation is part of the recorded geometry (the plain gather cannot execute it)."""
        return self.transposed or bool((self.ys == -2).any() or (self.xs == -2).any())

    def __getitem__(self, key):
        if self.resized is not None:
            raise TypeError("a resized lazy image is final")
        if not isinstance(key, tuple):
            key = (key,)
        if len(key) > 2 or not all(isinstance(k, slice) for k in key):
            raise TypeError("lazy images take row / column slices only")
        ys = self.ys[key[0]]
        xs = self.xs[key[1]] if len(key) > 1 else self.xs
        return GeoImage(ys, xs, self.background, transposed=self.transposed)

    def window(self, top, left, height, width, background):
        """CropPad's window (data_generator/object_detection_2d_patch_sampling_ops.py: the patch, background where it leaves the image)."""
        h, w = len(self.ys), len(self.xs)
        rows = np.arange(top, top + height)
        cols = np.arange(left, left + width)
        ys = np.where((rows >= 0) & (rows < h), self.ys[np.clip(rows, 0, h - 1)], -1)
        xs = np.where((cols >= 0) & (cols < w), self.xs[np.clip(cols, 0, w - 1)], -1)
        bg = tuple(int(v) for v in background)
        padded = bool(top < 0 or left < 0 or top + height > h or left + width > w)     # THIS window leaves the (virtual) image
        had = bool((self.ys == -1).any() or (self.xs == -1).any())
        if padded and had and self.background is not None and tuple(self.background) != bg:
            raise NotImplementedError("two paddings with different background colours cannot be composed lazily")
        return GeoImage(ys, xs, bg if (padded or self.background is None) else self.background, transposed=self.transposed)

    def turn(self, angle):
        """Rotate's warpAffine (object_detection_2d_geometric_ops.Rotate: the reference's adjusted matrix, border 0) as the exact index
        permutation it is: output pixel (row y, column x) of an H x W image reads (column, row) = (W - y, x) for 90 degrees, (W - x, H - y)
        for 180, (y, H - x) for 270; a position outside the image is black (-2)."""
        if self.resized is not None:
            raise TypeError("a resized lazy image is final")
        if (self.ys == -1).any() or (self.xs == -1).any():
            raise NotImplementedError("a rotation after a padding cannot be composed lazily")
        h, w = len(self.ys), len(self.xs)
        ys_back = np.append(self.ys, -2)[h - np.arange(h)]        # position k -> what sits at h - k (h itself: outside)
        xs_back = np.append(self.xs, -2)[w - np.arange(w)]
        if angle == 90:
            return GeoImage(xs_back, self.ys, self.background, transposed=not self.transposed)
        if angle == 180:
            return GeoImage(ys_back, xs_back, self.background, transposed=self.transposed)
        if angle == 270:
            return GeoImage(self.xs, ys_back, self.background, transposed=not self.transposed)
        raise NotImplementedError("lazy images rotate by 90, 180 or 270 degrees only")

    def warp(self, M, dsize, background):
        """cv2.warpAffine on a lazy image: only Rotate's three matrices for this image's size, with their output size and a black border,
        are index permutations (`turn`); anything else cannot be recorded."""
        if np.any(border_value(background, 3) != 0):
            raise NotImplementedError("lazy images take Rotate's warps (border 0) only")
        h, w = len(self.ys), len(self.xs)
        m = np.asarray(M, dtype=np.float64)
        for angle in (90, 180, 270):
            ref, size = quarter_turn_matrix(h, w, angle)
            if m.shape == (2, 3) and np.array_equal(m, ref) and (int(dsize[0]), int(dsize[1])) == size:
                return self.turn(angle)
        raise NotImplementedError("lazy images take Rotate's warps (90, 180, 270 degrees about the centre) only")

    def resize(self, out_h, out_w, interp):
        return GeoImage(self.ys, self.xs, self.background, resized=(int(out_h), int(out_w), int(interp)), transposed=self.transposed)

    def plan(self):
        """(kind, area, ix, wx, iy, wy) of the final resize (`resize_plan`), its tap indices composed with the index maps: a tap
        addresses a column / row of the ORIGINAL image (a row / column when `transposed`), or -1 = a position the expansion filled with
        the background colour, -2 = one a rotation left black."""
        out_h, out_w, interp = self.resized
        kind, ix, wx, iy, wy, area = resize_plan(len(self.ys), len(self.xs), out_h, out_w, interp)
        return kind, area, self.xs[ix].astype(np.int32), wx, self.ys[iy].astype(np.int32), wy


def _gather_tables(lazies, n_min):
    """The padded per-image tables of a batch of resized GeoImages: (kinds (B, 4), ix, wx, iy, wy, background (B, 3), transposed (B,) |
    None when no image has rotated, plans)."""
    plans = [l.plan() for l in lazies]
    n = max(max(pl[2].shape[1], pl[4].shape[1]) for pl in plans)
    n = max(n_min, 1 if n <= 1 else (2 if n <= 2 else (4 if n <= 4 else (8 if n <= 8 else 16 if n <= 16 else n))))
    b, (out_h, out_w) = len(lazies), lazies[0].resized[:2]
    ix, wx = np.zeros((b, out_w, n), dtype=np.int32), np.zeros((b, out_w, n), dtype=np.float64)
    iy, wy = np.zeros((b, out_h, n), dtype=np.int32), np.zeros((b, out_h, n), dtype=np.float64)
    kinds = np.zeros((b, 4), dtype=np.int32)                      # kind, area, taps per column, taps per row
    for k, (kind, area, sx, vx, sy, vy) in enumerate(plans):
        ix[k, :, :sx.shape[1]], wx[k, :, :sx.shape[1]] = sx, vx
        iy[k, :, :sy.shape[1]], wy[k, :, :sy.shape[1]] = sy, vy
        kinds[k] = (kind, area, sx.shape[1], sy.shape[1])
    bg = np.array([(l.background if l.background is not None else (0, 0, 0)) for l in lazies], dtype=np.uint8)
    turned = np.array([int(l.transposed) for l in lazies], dtype=np.int32) if any(l.turned for l in lazies) else None
    return kinds, ix, wx, iy, wy, bg, turned, plans


def gather_batch(images, lazies):
    """Execute the recorded geometry of a batch: images (B, H, W, 3) CUDA uint8, lazies[i] a resized GeoImage of image i -> the
    (B, out_h, out_w, 3) uint8 batch, ONE launch (every image with its own cv2.resize arithmetic: `kinds`)."""
    sizes = {l.resized[:2] for l in lazies}
    if len(sizes) != 1:
        raise ValueError("every image of a batch must end in the same size")
    out_h, out_w = sizes.pop()
    kinds, ix, wx, iy, wy, bg, turned, _ = _gather_tables(lazies, 1)
    if turned is not None:
        return nat.image_resize_gather_turn_u8(images.contiguous(), None, out_h, out_w, kinds, ix, wx, iy, wy, turned, bg)
    return nat.image_resize_gather_cv_u8(images.contiguous(), out_h, out_w, kinds, ix, wx, iy, wy, bg)


# ---- ragged batches: images of different sizes in one device buffer ----------------------------------------------------------------
RAGGED_ALIGN = 256                                           # byte alignment of every image in a ragged buffer


class RaggedBatch:
    """B uint8 images of different sizes on the device: `data` (a CUDA uint8 buffer), `table` ((B, 4) int64 CUDA tensor: byte offset into
    `data`, H, W, C), `shapes` (the B (H, W, C) on the host) and `max_pixels` (the largest H W)."""

    def __init__(self, data, table, shapes):
        self.data, self.table, self.shapes = data, table, [tuple(int(v) for v in s) for s in shapes]
        self.max_pixels = max(h * w for h, w, _ in self.shapes)

    def __len__(self):
        return len(self.shapes)

    def like(self, data):
        return RaggedBatch(data, self.table, self.shapes)


def _hwc(image):
    shape = tuple(int(v) for v in image.shape)
    if len(shape) == 2:
        return shape + (1,)
    if len(shape) == 3 and shape[2] in (1, 3, 4):
        return shape
    raise ValueError("a ragged batch takes (H, W) or (H, W, C) images with C in (1, 3, 4), not %s" % (shape,))


def pack_ragged(images, device=None):
    """A list of uint8 images (NumPy arrays or CUDA tensors, (H, W) or (H, W, C), C in 1 / 3 / 4) -> RaggedBatch.  Host images cross
    PCIe in ONE copy: [table | image 0 | image 1 | ...], each part starting on a RAGGED_ALIGN boundary."""
    import torch
    if len(images) == 0:
        raise ValueError("a ragged batch holds at least one image")
    shapes = [_hwc(im) for im in images]
    for im in images:
        if (im.dtype != np.uint8) if isinstance(im, np.ndarray) else (im.dtype != torch.uint8):
            raise TypeError("ragged batches hold uint8 images")
    B = len(images)
    head = -(-B * 32 // RAGGED_ALIGN) * RAGGED_ALIGN
    offsets, pos = [], 0
    for h, w, c in shapes:
        offsets.append(pos)
        pos += -(-h * w * c // RAGGED_ALIGN) * RAGGED_ALIGN
    table = np.array([(o, h, w, c) for o, (h, w, c) in zip(offsets, shapes)], dtype=np.int64)
    if device is None:
        dev = next((im.device for im in images if torch.is_tensor(im) and im.is_cuda), None)
        device = dev if dev is not None else torch.device("cuda", torch.cuda.current_device())
    host = np.zeros((head + pos,), dtype=np.uint8)
    host[:B * 32] = table.view(np.uint8).ravel()
    on_device = []
    for im, o, (h, w, c) in zip(images, offsets, shapes):
        if isinstance(im, np.ndarray):
            host[head + o:head + o + h * w * c] = np.ascontiguousarray(im).reshape(-1)
        else:
            on_device.append((im, o, h * w * c))
    buf = torch.from_numpy(host).to(device)
    for im, o, n in on_device:                               # device images: copied into place on the device
        buf[head + o:head + o + n].copy_(im.reshape(-1))
    return RaggedBatch(buf[head:], buf[:B * 32].view(torch.int64).view(B, 4), shapes)


def gather_batch_ragged(packed, lazies):
    """Execute the recorded geometry of a ragged batch: lazies[i] a resized GeoImage over image i (its index maps address image i's own
    rows / columns) -> the (B, out_h, out_w, 3) uint8 batch, ONE launch; 1- and 4-channel images are read as ConvertTo3Channels makes them."""
    sizes = {l.resized[:2] for l in lazies}
    if len(sizes) != 1:
        raise ValueError("every image of a batch must end in the same size")
    if len(lazies) != len(packed):
        raise ValueError("one lazy image per image of the batch")
    out_h, out_w = sizes.pop()
    kinds, ix, wx, iy, wy, bg, turned, plans = _gather_tables(lazies, 2)
    for l, (kind, area, sx, vx, sy, vy), (h, w, _) in zip(lazies, plans, packed.shapes):
        if sx.max() >= (h if l.transposed else w) or sy.max() >= (w if l.transposed else h):
            raise ValueError("the recorded geometry is not of these images")
    if turned is not None:
        return nat.image_resize_gather_turn_u8(packed.data, packed.table, out_h, out_w, kinds, ix, wx, iy, wy, turned, bg)
    return nat.image_resize_gather_ragged_u8(packed.data, packed.table, out_h, out_w, kinds, ix, wx, iy, wy, bg)


def run_ragged(packed, programs):
    """Per-image uint8 -> uint8 programs on a ragged batch of 3-channel images, ONE launch -> a RaggedBatch of the results."""
    if any(c != 3 for _, _, c in packed.shapes):
        raise ValueError("photometric programs take 3-channel images")
    for p in programs:
        if end_dtype(np.uint8, p) != U8:
            raise ValueError("a ragged program must end in uint8")
    enc = [encode(p) for p in programs]
    out = nat.image_program_ragged_u8(packed.data, packed.table, packed.max_pixels, np.stack([e[0] for e in enc]),
                                      np.stack([e[1] for e in enc]))
    return packed.like(out)


# ---- lazy geometry with ONE resampling stage: Translate / Scale in a composed list ----------------------------------------------------
class StagedGeoImage:
    """A `GeoImage` that can also hold ONE cv2.warpAffine in front of the final resize: index maps `a` over the original image, the
    `stage` (M float64 (2, 3), (out_h, out_w), border colour) over a's virtual image, and index maps `b` over the stage's output (with
    the final resize).  The 8-bit rounding of the warp is part of the result, so the stage is a pixel pass of its own
    (`warp_stage_ragged`: ssdhip_image_warp_affine_ragged_u8 into a ragged intermediate that the gather then reads through `b`).
    Without a stage it is `a` and behaves as a GeoImage does.  What `warp` records:
      * a translation by whole pixels that keeps the size (Translate; Scale(1)): under warpAffine's arithmetic an exact copy with the
        border colour where the canvas is uncovered = `window(-dy, -dx, h, w, border)` on the current maps;
      * Rotate's three matrices for the current size, border 0: `turn`, as GeoImage.warp;
      * the first other matrix: the stage, unless a quarter turn sits in front of it (the kernel's maps are not transposed);
      * a second one: NotImplementedError, like everything else the maps cannot hold (the generator then runs the per-image loop)."""

    ndim = 3
    dtype = np.dtype(np.uint8)

    def __init__(self, a, stage=None, b=None):
        self.a, self.stage, self.b = a, stage, b

    @classmethod
    def of(cls, height, width):
        return cls(GeoImage.of(height, width))

    @property
    def top(self):
        """The maps the next op applies to."""
        return self.a if self.stage is None else self.b

    def _on_top(self, maps):
        return StagedGeoImage(maps, None, None) if self.stage is None else StagedGeoImage(self.a, self.stage, maps)

    @property
    def shape(self):
        return self.top.shape

    @property
    def resized(self):
        return self.top.resized

    def __getitem__(self, key):
        return self._on_top(self.top[key])

    def window(self, top, left, height, width, background):
        return self._on_top(self.top.window(top, left, height, width, background))

    def turn(self, angle):
        return self._on_top(self.top.turn(angle))

    def resize(self, out_h, out_w, interp):
        return self._on_top(self.top.resize(out_h, out_w, interp))

    def warp(self, M, dsize, background):
        top = self.top
        if top.resized is not None:
            raise TypeError("a resized lazy image is final")
        h, w = len(top.ys), len(top.xs)
        out_w, out_h = int(dsize[0]), int(dsize[1])
        border = tuple(int(v) for v in border_value(background, 3))
        m = np.asarray(M, dtype=np.float64)
        if m.shape != (2, 3):
            raise ValueError("a warp matrix is (2, 3)")
        shift = _integer_shift(m)
        if shift is not None and (out_h, out_w) == (h, w):
            return self.window(-shift[1], -shift[0], h, w, border)
        if border == (0, 0, 0):
            for angle in (90, 180, 270):
                ref, size = quarter_turn_matrix(h, w, angle)
                if np.array_equal(m, ref) and (out_w, out_h) == size:
                    return self.turn(angle)
        if self.stage is not None:
            raise NotImplementedError("two non-integer warps cannot be composed lazily")
        if self.a.turned:
            raise NotImplementedError("a warp after a rotation cannot be composed lazily")
        if out_h < 1 or out_w < 1:
            raise ValueError("a warp's output has at least one pixel")
        return StagedGeoImage(self.a, (m.copy(), (out_h, out_w), border), GeoImage.of(out_h, out_w))


def _rgb_word(colour):
    r, g, b = (int(v) for v in colour)
    return r | (g << 8) | (b << 16)


def warp_stage_ragged(packed, geos):
    """The stages of a batch of final StagedGeoImages over a ragged batch: ONE ssdhip_image_warp_affine_ragged_u8 launch into a fresh
    ragged buffer of 3-channel images -> (that RaggedBatch, the GeoImages over ITS images for `gather_batch_ragged`).  An image without
    a stage goes through the launch with identity tables and identity maps -- fx = fy = 0 gives the weight 32768, an exact copy, made
    3-channel as the gather would read it -- and keeps its maps (they may hold a quarter turn, which the warp's maps cannot; the gather
    executes it as ever).  The tables of the batch go up as one array."""
    if len(geos) != len(packed):
        raise ValueError("one lazy image per image of the batch")
    parts, meta, out_table, out_shapes, after, pos, out_pos = [], [], [], [], [], 0, 0
    for g, (h, w, _) in zip(geos, packed.shapes):
        if g.stage is None:
            xs, ys, M, (out_h, out_w), border, padding = np.arange(w), np.arange(h), _IDENTITY, (h, w), (0, 0, 0), (0, 0, 0)
            after.append(g.a)
        else:
            M, (out_h, out_w), border = g.stage
            xs, ys, padding = g.a.xs, g.a.ys, (g.a.background if g.a.background is not None else (0, 0, 0))
            after.append(g.b)
        xtab, ytab = warp_tables(M, out_h, out_w)
        row = []
        for part in (xtab, ytab, xs, ys):
            part = np.asarray(part, dtype=np.int32).reshape(-1)
            row.append(pos)
            parts.append(part)
            pos += part.size
        meta.append(row + [len(xs), len(ys), _rgb_word(border), _rgb_word(padding)])
        out_table.append((out_pos, out_h, out_w, 3))
        out_shapes.append((out_h, out_w, 3))
        out_pos += -(-out_h * out_w * 3 // RAGGED_ALIGN) * RAGGED_ALIGN
    data, table = nat.image_warp_affine_ragged_u8(packed.data, packed.table, packed.shapes, np.array(out_table, dtype=np.int64), out_pos,
                                                  np.concatenate(parts), np.array(meta, dtype=np.int32))
    return RaggedBatch(data, table, out_shapes), after


# ---- lazy photometry: the photometric ops of a composed list recorded around the recorded geometry ------------------------------------
class ProgramImage:
    """An image that exists only as WHAT A TRANSFORMATION LIST DID TO IT: the photometric steps in front of the geometry (`pre`), the
    geometry (a `GeoImage`; a `StagedGeoImage` when made with `warps=True`), and the photometric steps behind it (`post`) -- executed
    for a whole batch by `run_program_batch`.  Steps are the (name, argument) pairs of `encode` plus two that need a table: ("gamma", table) = cv2.LUT with a 256-entry uint8 table on all
    three channels, ("equalize", channel) = cv2.equalizeHist on one channel.  Quacks like the array the ops expect: `shape`, `ndim` and
    row / column slicing are the GeoImage's, `dtype` is what the recorded steps leave (`end_dtype`), `image[:, :, order]` is ChannelSwap.
    What a NumPy image of that dtype would refuse is refused when it is recorded, with the same exception; what cannot be composed --
    geometry on a state that is not uint8 or behind a step of `post`, more than 15 steps or four tables in a segment -- raises
    NotImplementedError (the generator then runs the per-image loop)."""

    ndim = 3

    def __init__(self, geo, pre=(), post=(), moved=False):
        self.geo, self.pre, self.post, self.moved = geo, list(pre), list(post), bool(moved)

    @classmethod
    def of(cls, height, width, warps=False):
        """`warps`: the geometry is a `StagedGeoImage`, which also records Translate / Scale (below, behind cv2.warpAffine's tables)."""
        return cls(StagedGeoImage.of(height, width) if warps else GeoImage.of(height, width))

    @property
    def shape(self):
        return self.geo.shape

    @property
    def dtype(self):
        return np.dtype(end_dtype(end_dtype(U8, self.pre), self.post))

    def record(self, steps):
        """The image after `steps`: appended to the segment in front of the geometry while no geometric op has been recorded, else behind it."""
        tag = str(self.dtype)
        segment = list(self.post if self.moved else self.pre)
        for name, arg in steps:
            if name == "gamma":
                if tag != U8:
                    raise TypeError("look-up tables apply to uint8 images")
                arg = np.asarray(arg, dtype=np.uint8).reshape(256)
            elif name == "equalize":
                if tag != U8:
                    raise TypeError("histogram equalisation takes uint8 images")
                if int(arg) not in (0, 1, 2):
                    raise ValueError("a channel is 0, 1 or 2")
            else:
                nat.IMG_OPS[name]
            tag = end_dtype(tag, [(name, arg)])
            segment.append((name, arg))
        if len(segment) > nat.IMG_PROG - 1:
            raise NotImplementedError("a recorded segment holds at most %d steps" % (nat.IMG_PROG - 1))
        if sum(name in ("gamma", "equalize") for name, _ in segment) > nat.IMG_LUT_SLOTS:
            raise NotImplementedError("a recorded segment holds at most %d look-up tables" % nat.IMG_LUT_SLOTS)
        return ProgramImage(self.geo, self.pre, segment, True) if self.moved else ProgramImage(self.geo, segment)

    def _geometry(self, geo_of):
        if self.post:
            raise NotImplementedError("geometry behind the second photometric segment cannot be composed lazily")
        if self.dtype != np.uint8:
            raise NotImplementedError("the recorded geometry takes uint8 images")
        return ProgramImage(geo_of(self.geo), self.pre, (), True)

    def __getitem__(self, key):
        full = slice(None, None, None)
        if isinstance(key, tuple) and len(key) == 3 and key[0] == full and key[1] == full and isinstance(key[2], (tuple, list, np.ndarray)):
            return self.record([("swap", swap_code(key[2]))])                 # ChannelSwap: image[:, :, order]
        if not all(isinstance(k, slice) for k in (key if isinstance(key, tuple) else (key,))):
            raise NotImplementedError("lazy images take row / column slices and channel orders only")
        return self._geometry(lambda geo: geo[key])

    def window(self, top, left, height, width, background):
        return self._geometry(lambda geo: geo.window(top, left, height, width, background))

    def warp(self, M, dsize, background):
        return self._geometry(lambda geo: geo.warp(M, dsize, background))

    def resize(self, out_h, out_w, interp):
        return self._geometry(lambda geo: geo.resize(out_h, out_w, interp))


def _segment_tables(programs):
    """A batch's recorded segments -> (the encodable programs: every table step as ("lut", slot + 4 mask), the slots dealt in step order;
    the gamma tables in their slots, (B, 4, 256) uint8; per image its equalize steps [(position, channel, slot), ...]; tables used?)."""
    luts = np.zeros((len(programs), nat.IMG_LUT_SLOTS, 256), dtype=np.uint8)
    plain, equalizes, used = [], [], False
    for i, program in enumerate(programs):
        steps, eq, slot = [], [], 0
        for k, (name, arg) in enumerate(program):
            if name == "gamma":
                luts[i, slot] = arg
                steps.append(("lut", slot + 4 * 7))
            elif name == "equalize":
                eq.append((k, int(arg), slot))
                steps.append(("lut", slot + 4 * (1 << int(arg))))
            else:
                steps.append((name, arg))
                continue
            slot += 1
        used = used or slot > 0
        plain.append(steps)
        equalizes.append(eq)
    return plain, luts, equalizes, used


def _run_segment(programs, device, launch_program, launch_hist):
    """One recorded segment of a batch (every image on a uint8 state): without tables ONE launch (`launch_program(ops, args, None)`); with
    them the gamma tables go up once, every equalize position costs one histogram launch over the programs' prefixes
    (`launch_hist(ops, args, luts, stop, channel, hist)`) and one table launch, then `launch_program(ops, args, luts)`."""
    plain, luts_host, equalizes, used = _segment_tables(programs)
    enc = [encode(p) for p in plain]
    ops, args = np.stack([e[0] for e in enc]), np.stack([e[1] for e in enc])
    if not used:
        return launch_program(ops, args, None)
    import torch
    nat.image_program_check(ops, args, nat.IMG_U8, True)
    ops, args = nat.to_device(ops, device=device, dtype=torch.int32), nat.to_device(args, device=device, dtype=torch.float64)
    luts = nat.to_device(luts_host, device=device)
    hist = None
    for level in range(max(len(eq) for eq in equalizes)):
        sel = np.full((3, len(programs)), -1, dtype=np.int32)              # stop, channel, slot
        sel[1] = 0
        for i, eq in enumerate(equalizes):
            if len(eq) > level:
                sel[:, i] = eq[level]
        hist = launch_hist(ops, args, luts, sel[0], sel[1], hist)
        nat.image_equalize_tables(hist, sel[2], luts)
    return launch_program(ops, args, luts)


def _three_channels(image):
    """ConvertTo3Channels (object_detection_2d_photometric_ops): grey replicated, alpha dropped."""
    if image.ndim == 2:
        return np.stack([image] * 3, axis=-1)
    if image.shape[2] == 1:
        return np.concatenate([image] * 3, axis=-1)
    return image[:, :, :3]


def run_program_batch(images, lazies):
    """Execute a batch of ProgramImages over the uint8 host images they were recorded for -> the CUDA batch (B, H, W, 3), uint8, float32 or
    float64 as the programs end.  First segments on the ragged batch (nothing is launched when all are empty; 1- and 4-channel images are
    made 3-channel on the host when one is not), then the ragged gather (a copy-kind plan for a list without a resize: every image must
    end in one size), then the second segments on the gather's output.  NotImplementedError for sizes or dtypes that differ.  When an image
    of the batch carries a warp stage (`StagedGeoImage`), ONE warp launch for the whole batch sits between the first segments and the
    gather (`warp_stage_ragged`); a batch without a stage takes exactly the launches above."""
    import torch
    if len(images) != len(lazies) or not lazies:
        raise ValueError("one lazy image per image of the batch")
    pres, posts, geos = [], [], []
    for l in lazies:
        pre, post = list(l.pre), list(l.post)
        if not l.moved and end_dtype(U8, pre) != U8:                          # no geometry at all: the steps may as well follow it
            pre, post = [], pre
        if end_dtype(U8, pre) != U8:
            raise NotImplementedError("the recorded geometry takes uint8 images")
        pres.append(pre)
        posts.append(post)
        geos.append(l.geo if l.geo.resized is not None else l.geo.resize(l.geo.shape[0], l.geo.shape[1], INTER_NEAREST))
    if len({g.resized[:2] for g in geos}) != 1:
        raise NotImplementedError("every image of a batch must end in the same size")
    tags = {end_dtype(U8, p) for p in posts}
    if len(tags) != 1:
        raise NotImplementedError("the programs of a batch must end in the same dtype")
    if any(pres):
        images = [im if (im.ndim == 3 and im.shape[2] == 3) else _three_channels(im) for im in images]
    packed = pack_ragged(images)
    device = packed.data.device
    if any(pres):
        packed = packed.like(_run_segment(
            pres, device,
            lambda ops, args, luts: nat.image_program_ragged_u8(packed.data, packed.table, packed.max_pixels, ops, args, luts),
            lambda ops, args, luts, stop, channel, hist: nat.image_program_hist_u8(packed.data, packed.table, packed.max_pixels, ops, args,
                                                                                 luts, stop, channel, hist)))
    if any(isinstance(g, StagedGeoImage) and g.stage is not None for g in geos):
        packed, geos = warp_stage_ragged(packed, [g if isinstance(g, StagedGeoImage) else StagedGeoImage(g) for g in geos])
    else:                                                                     # no stage in the batch: the launches of a list without warps
        geos = [g.a if isinstance(g, StagedGeoImage) else g for g in geos]
    out = gather_batch_ragged(packed, geos)
    if any(posts):
        out_dtype = _torch_dtype(tags.pop())
        out = _run_segment(
            posts, device,
            lambda ops, args, luts: nat.image_program(out, ops, args, out_dtype, luts),
            lambda ops, args, luts, stop, channel, hist: nat.image_program_hist_u8(out, None, 0, ops, args, luts, stop, channel, hist))
    return out


# ---- cv2.resize for 8-bit images: the tables of OpenCV's imgproc/resize.cpp (3.4 / 4.x), the arithmetic runs in csrc/ssdhip_image.hip ----
# cv::resize on CV_8U (round 6; the first version resampled with float64 weights and one rounding, off by one grey level here and there):
#   LINEAR / CUBIC / LANCZOS4, and AREA when an axis grows ("area_mode" bilinear): per output column / row the float32 kernel values become
#     11-bit fixed-point `short`s (saturate_cast<short>(c * 2048), nearest-even); rows are int32 sums of uchar x short; the vertical pass is
#     uchar((((b0 (S0 >> 4)) >> 16) + ((b1 (S1 >> 4)) >> 16) + 2) >> 2) for the linear kernel and saturate((sum + 2^21) >> 22) for the
#     4- and 8-tap ones.  Columns reset (sx, fx) at the borders for the linear kernel; rows are clamped with their coefficients kept;
#   AREA with both scales >= 1: integer scales -> block sums, saturate(cvRound(sum * (1.f / area))), the 2 x 2 block (sum + 2) >> 2 (also
#     what INTER_LINEAR does at exactly 2 x 2); otherwise computeResizeAreaTab's float32 alpha / beta accumulated in float32, cvRound;
#   NEAREST: min(floor(dst * (1 / (n_dst / n_src))), n_src - 1); equal sizes: a copy.
# A plan = (kind, ix, wx, iy, wy, area): tap indices and the table values as float64 (shorts / float32 alphas / ones are all exact there).
INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA, INTER_LANCZOS4 = 0, 1, 2, 3, 4
KIND_NEAREST, KIND_LINEAR, KIND_KERNEL, KIND_AREA, KIND_AREA_FAST, KIND_AREA_FAST2, KIND_COPY = 0, 1, 2, 3, 4, 5, 6
COEF_SCALE = 2048                                           # 1 << INTER_RESIZE_COEF_BITS
_f32 = np.float32
_PI = 3.1415926535897932384626433832795                     # CV_PI


def _scales(n_src, n_dst):
    inv = float(n_dst) / float(n_src)                       # inv_scale = (double)dsize / ssize;  scale = 1. / inv_scale
    return inv, 1.0 / inv


def _to_short(coef):
    """saturate_cast<short>(float32 coefficient * 2048): nearest-even, clamped."""
    v = np.asarray(coef, dtype=_f32) * _f32(COEF_SCALE)
    return np.clip(np.rint(v.astype(np.float64)), -32768, 32767)


def _kernel_cubic(x):
    """interpolateCubic, A = -0.75, every operation in float32: (n,) -> (n, 4)."""
    x = np.asarray(x, dtype=_f32)
    a = _f32(-0.75)
    u = x + _f32(1)
    c0 = ((a * u - _f32(5) * a) * u + _f32(8) * a) * u - _f32(4) * a
    c1 = ((a + _f32(2)) * x - (a + _f32(3))) * x * x + _f32(1)
    v = _f32(1) - x
    c2 = ((a + _f32(2)) * v - (a + _f32(3))) * v * v + _f32(1)
    return np.stack([c0, c1, c2, _f32(1) - c0 - c1 - c2], axis=1).astype(_f32)


import math as _math
_INV_FACT = [1.0 / _math.factorial(_k) for _k in range(24)]      # exact integers, ONE rounding each (the literals of csrc/ssdhip_augment.hip)


def sincos_near_minus_pi(y):
    """(sin y, cos y) for y in [-pi, -3 pi / 4] by a FIXED chain of float64 operations (t = y + pi; Taylor polynomials of degree 23 / 22 in
    Horner form, signs folded into the subtractions): the GPU runs the same chain (csrc/ssdhip_augment.hip), so host- and device-built
    Lanczos tables agree to the bit.  Within 1 ulp of the C library's."""
    t = np.asarray(y, dtype=np.float64) + _PI
    t2 = t * t
    s = np.full_like(t2, _INV_FACT[23])
    for k in range(21, 0, -2):
        s = _INV_FACT[k] - s * t2
    c = np.full_like(t2, _INV_FACT[22])
    for k in range(20, -1, -2):
        c = _INV_FACT[k] - c * t2
    return -(s * t), -c


def _kernel_lanczos4(x):
    """interpolateLanczos4: (n,) float32 -> (n, 8) float32."""
    x = np.asarray(x, dtype=_f32).reshape(-1)
    r = 0.70710678118654752440084436210485
    cs = ((1, 0), (-r, -r), (0, 1), (r, -r), (-1, 0), (r, r), (0, -1), (-r, r))
    out = np.zeros((x.shape[0], 8), dtype=_f32)
    centre = x < np.finfo(_f32).eps                           # x < FLT_EPSILON
    out[centre, 3] = 1
    rest = ~centre
    if rest.any():
        x3 = x[rest] + _f32(3)
        s0, c0 = sincos_near_minus_pi(-(x3.astype(np.float64)) * _PI * 0.25)
        co = np.empty((x3.shape[0], 8), dtype=_f32)
        for i in range(8):
            y = -((x3 - _f32(i)).astype(np.float64)) * _PI * 0.25
            co[:, i] = ((cs[i][0] * s0 + cs[i][1] * c0) / (y * y)).astype(_f32)
        total = np.zeros(x3.shape[0], dtype=_f32)
        for i in range(8):
            total = total + co[:, i]
        out[rest] = co * (_f32(1) / total)[:, None]
    return out


def _coords(n_src, n_dst, area_mode):
    """(sx, fx) per destination coordinate before the border rules: fx = (float)((d + 0.5) scale - 0.5), or the area-mode variant."""
    inv, scale = _scales(n_src, n_dst)
    d = np.arange(n_dst, dtype=np.float64)
    if area_mode:
        sx = np.floor(d * scale).astype(np.int64)
        fx = ((d + 1) - (sx + 1) * inv).astype(_f32)
        return sx, np.where(fx <= 0, _f32(0), fx - np.floor(fx)).astype(_f32)
    fx = ((d + 0.5) * scale - 0.5).astype(_f32)
    sx = np.floor(fx).astype(np.int64)
    return sx, (fx - sx.astype(_f32)).astype(_f32)


def fixed_axis(n_src, n_dst, interp, area_mode, horizontal):
    """Tap indices (n_dst, k) int32 and `short` coefficients (n_dst, k) float64 of one axis of the fixed-point paths."""
    sx, fx = _coords(n_src, n_dst, area_mode)
    if interp in (INTER_LINEAR, INTER_AREA):
        if horizontal:
            lo, hi = sx < 0, sx >= n_src - 1
            fx = np.where(lo | hi, _f32(0), fx).astype(_f32)
            sx = np.where(lo, 0, np.where(hi, n_src - 1, sx))
        offs, coef = np.array([0, 1]), np.stack([_f32(1) - fx, fx], axis=1)
    elif interp == INTER_CUBIC:
        offs, coef = np.array([-1, 0, 1, 2]), _kernel_cubic(fx)
    elif interp == INTER_LANCZOS4:
        offs, coef = np.arange(-3, 5), _kernel_lanczos4(fx)
    else:
        raise ValueError("interpolation mode %r is not one of cv2's INTER_NEAREST .. INTER_LANCZOS4 (0 .. 4)" % (interp,))
    return np.clip(sx[:, None] + offs[None, :], 0, n_src - 1).astype(np.int32), _to_short(coef)


def area_axis(n_src, n_dst):
    """computeResizeAreaTab as padded per-destination taps: indices (n_dst, T) int32, float32 alphas (n_dst, T) as float64, zeros behind a
    row's own entries."""
    _, scale = _scales(n_src, n_dst)
    d = np.arange(n_dst, dtype=np.float64)
    f1 = d * scale
    f2 = f1 + scale
    cell = np.minimum(scale, n_src - f1)
    s2 = np.minimum(np.floor(f2).astype(np.int64), n_src - 1)
    s1 = np.minimum(np.ceil(f1).astype(np.int64), s2)
    head = (s1 - f1) > 1e-3
    tail = (f2 - s2) > 1e-3
    count = head.astype(np.int64) + (s2 - s1) + tail.astype(np.int64)
    T = max(1, int(count.max()))
    idx = np.zeros((n_dst, T), dtype=np.int64)
    alpha = np.zeros((n_dst, T), dtype=_f32)
    pos = np.arange(T)[None, :]
    first = (s1 - head.astype(np.int64))[:, None]                     # the row's first source index
    idx[:] = first + pos
    alpha[:] = (1.0 / cell)[:, None].astype(_f32)
    head_val = ((s1 - f1) / cell).astype(_f32)
    tail_val = (np.minimum(np.minimum(f2 - s2, 1.0), cell) / cell).astype(_f32)
    alpha[head, 0] = head_val[head]
    rows = np.nonzero(tail)[0]
    alpha[rows, count[rows] - 1] = tail_val[rows]
    beyond = pos >= count[:, None]
    alpha[beyond] = 0
    last = np.take_along_axis(idx, np.maximum(count - 1, 0)[:, None], axis=1)
    idx = np.where(beyond, last, idx)
    return np.clip(idx, 0, n_src - 1).astype(np.int32), alpha.astype(np.float64)


def resize_plan(src_h, src_w, dst_h, dst_w, interp):
    """cv::resize's dispatch for these sizes -> (kind, ix, wx, iy, wy, area)."""
    interp = int(interp)
    if interp not in (INTER_NEAREST, INTER_LINEAR, INTER_CUBIC, INTER_AREA, INTER_LANCZOS4):
        raise ValueError("interpolation mode %r is not one of cv2's INTER_NEAREST .. INTER_LANCZOS4 (0 .. 4)" % (interp,))
    ones = lambda i: np.ones(i.shape, dtype=np.float64)
    if (src_h, src_w) == (dst_h, dst_w):
        ix, iy = np.arange(dst_w, dtype=np.int32)[:, None], np.arange(dst_h, dtype=np.int32)[:, None]
        return KIND_COPY, ix, ones(ix), iy, ones(iy), 1
    if interp == INTER_NEAREST:
        tabs = []
        for n_src, n_dst in ((src_w, dst_w), (src_h, dst_h)):
            i = np.minimum(np.floor(np.arange(n_dst, dtype=np.float64) * _scales(n_src, n_dst)[1]), n_src - 1).astype(np.int32)[:, None]
            tabs += [i, ones(i)]
        return (KIND_NEAREST,) + tuple(tabs) + (1,)
    scale_x, scale_y = _scales(src_w, dst_w)[1], _scales(src_h, dst_h)[1]
    isx, isy = int(np.rint(scale_x)), int(np.rint(scale_y))
    eps = np.finfo(np.float64).eps
    fast = abs(scale_x - isx) < eps and abs(scale_y - isy) < eps
    if interp == INTER_LINEAR and fast and isx == 2 and isy == 2:
        interp = INTER_AREA
    if interp == INTER_AREA and scale_x >= 1 and scale_y >= 1:
        if fast:
            ix = (np.arange(dst_w)[:, None] * isx + np.arange(isx)[None, :]).astype(np.int32)
            iy = (np.arange(dst_h)[:, None] * isy + np.arange(isy)[None, :]).astype(np.int32)
            return (KIND_AREA_FAST2 if (isx, isy) == (2, 2) else KIND_AREA_FAST), ix, ones(ix), iy, ones(iy), isx * isy
        ix, ax = area_axis(src_w, dst_w)
        iy, ay = area_axis(src_h, dst_h)
        return KIND_AREA, ix, ax, iy, ay, 1
    area_mode = interp == INTER_AREA
    ix, cx = fixed_axis(src_w, dst_w, interp, area_mode, True)
    iy, cy = fixed_axis(src_h, dst_h, interp, area_mode, False)
    return (KIND_LINEAR if interp in (INTER_LINEAR, INTER_AREA) else KIND_KERNEL), ix, cx, iy, cy, 1


def resize(image, out_h, out_w, interp):
    """cv2.resize(image, dsize=(out_w, out_h), interpolation=interp) for uint8 images: NumPy (H, W[, C]) or CUDA (B, H, W, C)."""
    if isinstance(image, (GeoImage, StagedGeoImage, ProgramImage)):
        return image.resize(out_h, out_w, interp)
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise TypeError("resize takes uint8 images")
        src = image if image.ndim == 3 else image[:, :, None]
        kind, ix, wx, iy, wy, area = resize_plan(src.shape[0], src.shape[1], out_h, out_w, interp)
        out = nat.image_resize_cv_u8(nat.to_device(np.ascontiguousarray(src)[None]), out_h, out_w, kind, area, ix, wx, iy, wy)[0].cpu().numpy()
        return out if image.ndim == 3 else out[:, :, 0]
    kind, ix, wx, iy, wy, area = resize_plan(int(image.shape[1]), int(image.shape[2]), out_h, out_w, interp)
    return nat.image_resize_cv_u8(image.contiguous(), out_h, out_w, kind, area, ix, wx, iy, wy)


# ---- cv2.LUT / cv2.equalizeHist ----------------------------------------------------------------------------------------------------
def lut(image, table, channel_mask):
    if isinstance(image, ProgramImage):
        if (int(channel_mask) & 7) != 7:
            raise NotImplementedError("lazy images take tables for all three channels only")
        return image.record([("gamma", table)])
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise TypeError("look-up tables apply to uint8 images")
        return nat.image_lut_u8(nat.to_device(np.ascontiguousarray(image)), np.asarray(table, dtype=np.uint8), channel_mask).cpu().numpy()
    return nat.image_lut_u8(image.contiguous(), np.asarray(table, dtype=np.uint8), channel_mask)


def equalize_table(hist):
    """cv2.equalizeHist's table from a 256-bin histogram: bins up to the first occupied one map to 0, the rest to the cumulative
    count scaled to 255 (float32 scale, rounded to nearest even); a constant plane is left alone."""
    hist = np.asarray(hist, dtype=np.int64)
    total = int(hist.sum())
    occupied = np.nonzero(hist)[0]
    if occupied.size == 0 or hist[occupied[0]] == total:
        return np.arange(256, dtype=np.uint8)
    first = int(occupied[0])
    scale = np.float32(255.0) / np.float32(total - hist[first])
    below = np.cumsum(hist) - hist[first]
    below[:first + 1] = 0
    return np.clip(np.rint((below.astype(np.float32) * scale).astype(np.float32)), 0, 255).astype(np.uint8)


def equalize_channel(image, channel):
    """image with cv2.equalizeHist applied to one channel (uint8; NumPy (H, W, C), one CUDA image (H, W, C), or a `ProgramImage`: recorded)."""
    if isinstance(image, ProgramImage):
        return image.record([("equalize", channel)])
    if isinstance(image, np.ndarray):
        if image.dtype != np.uint8:
            raise TypeError("histogram equalisation takes uint8 images")
        dev = nat.to_device(np.ascontiguousarray(image))
        table = equalize_table(nat.image_hist_u8(dev, channel).cpu().numpy())
        return nat.image_lut_u8(dev, table, 1 << channel).cpu().numpy()
    table = equalize_table(nat.image_hist_u8(image.contiguous(), channel).cpu().numpy())
    return nat.image_lut_u8(image.contiguous(), table, 1 << channel)


# ---- cv2.warpAffine for 8-bit images: OpenCV 3.4 / 4.x up to 4.10 (imgproc/imgwarp.cpp), the arithmetic runs in csrc/ssdhip_warp.hip ----
# (4.11 moved warpAffine to float arithmetic; the reference predates it.)  INTER_LINEAR, BORDER_CONSTANT only -- every call the reference
# makes (object_detection_2d_geometric_ops.py:287-291, 497-501, 703-705).  Without WARP_INVERSE_MAP the float64 matrix is inverted first
# (D = 1 / (M0 M4 - M1 M3), ...); then per column adelta = cvRound(M0 x 1024), bdelta = cvRound(M3 x 1024), per row
# X0 = cvRound((M1 y + M2) 1024) + 16, Y0 = cvRound((M4 y + M5) 1024) + 16, and the device does X = (X0 + adelta) >> 5, sx = X >> 5,
# fx = X & 31 and remapBilinear's 15-bit weights 32 (32 - fx)(32 - fy), ... which sum to 32768 (the table fix-up never fires).
def rotation_matrix_2d(center, angle, scale):
    """cv2.getRotationMatrix2D: `center` is a Point2f (float32 coordinates), `angle *= CV_PI / 180`, float64 result (2, 3)."""
    cx, cy = float(np.float32(center[0])), float(np.float32(center[1]))
    rad = float(angle) * (_PI / 180)
    a = _math.cos(rad) * float(scale)
    b = _math.sin(rad) * float(scale)
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], dtype=np.float64)


def quarter_turn_matrix(height, width, angle):
    """Rotate's adjusted matrix for a height x width image and its output size (width, height): getRotationMatrix2D about the centre, the
    translation moved by half the change of size (object_detection_2d_geometric_ops.Rotate, the reference :693-705)."""
    M = rotation_matrix_2d((width / 2, height / 2), angle, 1)
    cos_angle, sin_angle = np.abs(M[0, 0]), np.abs(M[0, 1])
    width_new = int(height * sin_angle + width * cos_angle)
    height_new = int(height * cos_angle + width * sin_angle)
    M[1, 2] += (height_new - height) / 2
    M[0, 2] += (width_new - width) / 2
    return M, (width_new, height_new)


def invert_affine(M):
    """warpAffine's in-place inversion of the (float64-widened) forward matrix -> the six coefficients of the inverse map."""
    m = [float(v) for v in np.asarray(M, dtype=np.float64).reshape(6)]
    d = m[0] * m[4] - m[1] * m[3]
    d = 1.0 / d if d != 0 else 0.0
    a11, a22 = m[4] * d, m[0] * d
    m[0], m[1], m[3], m[4] = a11, m[1] * -d, m[3] * -d, a22
    b1 = -m[0] * m[2] - m[1] * m[5]
    b2 = -m[3] * m[2] - m[4] * m[5]
    m[2], m[5] = b1, b2
    return m


def warp_tables(M, out_h, out_w):
    """(xtab (out_w, 2), ytab (out_h, 2)) int32: (adelta, bdelta) per column and (X0, Y0) per row of the forward matrix M."""
    m = invert_affine(M)
    x = np.arange(out_w, dtype=np.float64)
    y = np.arange(out_h, dtype=np.float64)
    xtab = np.stack([np.rint(m[0] * x * 1024.0), np.rint(m[3] * x * 1024.0)], axis=1)
    ytab = np.stack([np.rint((m[1] * y + m[2]) * 1024.0) + 16, np.rint((m[4] * y + m[5]) * 1024.0) + 16], axis=1)
    return xtab.astype(np.int32), ytab.astype(np.int32)


def border_value(background, channels):
    """saturate_cast<uchar> of a cv::Scalar's first `channels` entries (missing entries are 0)."""
    v = list(background) if isinstance(background, (list, tuple, np.ndarray)) else [background]
    v = (v + [0, 0, 0, 0])[:channels]
    return np.array([min(max(int(np.rint(float(a))), 0), 255) for a in v], dtype=np.uint8)


_IDENTITY = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def _integer_shift(M):
    """(dx, dy) when M is a translation by whole pixels (an exact copy under warpAffine's arithmetic), else None."""
    m = np.asarray(M, dtype=np.float64).reshape(2, 3)
    if m[0, 0] == 1 and m[0, 1] == 0 and m[1, 0] == 0 and m[1, 1] == 1 and float(m[0, 2]).is_integer() and float(m[1, 2]).is_integer():
        return int(m[0, 2]), int(m[1, 2])
    return None


class WarpImage:
    """An image that exists only as a recorded geometry over an image resident on the device (like `GeoImage`): at most one non-integer
    warp (`M`, its output size), integer translations before it (`pre`) and after it (`post`), and a horizontal flip at the end
    (`[:, ::-1]`) -- what Translate / Scale / Rotate / RandomFlip do to it, executed once for a whole batch by `warp_batch`
    (ssdhip_image_warp_affine_u8).  Anything else raises NotImplementedError."""

    ndim = 3
    dtype = np.dtype(np.uint8)

    def __init__(self, height, width, src_h=None, src_w=None, M=None, pre=(0, 0), post=None, flip=False, background=None):
        self.height, self.width = int(height), int(width)
        self.src_h = self.height if src_h is None else int(src_h)
        self.src_w = self.width if src_w is None else int(src_w)
        self.M, self.pre, self.post, self.flip, self.background = M, tuple(pre), post, bool(flip), background

    @classmethod
    def of(cls, height, width):
        return cls(height, width)

    @property
    def shape(self):
        return (self.height, self.width, 3)

    def _with(self, **kw):
        d = dict(height=self.height, width=self.width, src_h=self.src_h, src_w=self.src_w, M=self.M, pre=self.pre, post=self.post,
                 flip=self.flip, background=self.background)
        d.update(kw)
        return WarpImage(**d)

    def _bg(self, background):
        bg = tuple(int(v) for v in border_value(background, 3))
        if self.background is not None and self.background != bg:
            raise NotImplementedError("two warps with different background colours cannot be composed lazily")
        return bg

    def warp(self, M, dsize, background):
        """cv2.warpAffine(self, M, dsize, borderMode=BORDER_CONSTANT, borderValue=background), recorded."""
        out_w, out_h = int(dsize[0]), int(dsize[1])
        if self.flip or self.post is not None:
            raise NotImplementedError("a warp after a flip or after a second translation cannot be composed lazily")
        bg = self._bg(background)
        shift = _integer_shift(M)
        if shift is not None and (out_h, out_w) == (self.height, self.width):
            if self.M is None and self.pre == (0, 0):
                return self._with(pre=shift, background=bg)
            if self.M is None:
                return self._with(M=_IDENTITY, post=shift, background=bg)
            return self._with(post=shift, background=bg)
        if self.M is not None:
            raise NotImplementedError("two non-integer warps cannot be composed lazily")
        if self.pre != (0, 0) and (out_h, out_w) != (self.height, self.width):
            raise NotImplementedError("a translation before a warp that changes the image size cannot be composed lazily")
        return self._with(height=out_h, width=out_w, M=np.asarray(M, dtype=np.float64).reshape(2, 3), background=bg)

    def __getitem__(self, key):
        if not isinstance(key, tuple):
            key = (key,)
        full = slice(None, None, None)
        if len(key) == 2 and key[0] == full and key[1] == slice(None, None, -1) and not self.flip:
            return self._with(flip=True)
        raise NotImplementedError("lazy warped images take one horizontal flip ([:, ::-1]) only")

    def plan(self):
        """(geo (5,) int32, xtab, ytab, background (3,) uint8) of this image for ssdhip_image_warp_affine_u8."""
        xtab, ytab = warp_tables(_IDENTITY if self.M is None else self.M, self.height, self.width)
        post = self.post or (0, 0)
        geo = np.array([int(self.flip), self.pre[0], self.pre[1], post[0], post[1]], dtype=np.int32)
        bg = np.array(self.background if self.background is not None else (0, 0, 0), dtype=np.uint8)
        return geo, xtab, ytab, bg


def warp_batch(images, lazies):
    """Execute the recorded geometry of a batch: images (B, H, W, 3) CUDA uint8, lazies[i] a `WarpImage` of image i -> the
    (B, out_h, out_w, 3) uint8 batch, ONE launch."""
    sizes = {(l.height, l.width) for l in lazies}
    if len(sizes) != 1:
        raise ValueError("every image of a batch must end in the same size")
    if any((l.src_h, l.src_w) != (int(images.shape[1]), int(images.shape[2])) for l in lazies):
        raise ValueError("the recorded geometry is not of these images")
    out_h, out_w = sizes.pop()
    plans = [l.plan() for l in lazies]
    return nat.image_warp_affine_u8(images.contiguous(), out_h, out_w, np.stack([p[0] for p in plans]), np.stack([p[1] for p in plans]),
                                    np.stack([p[2] for p in plans]), np.stack([p[3] for p in plans]))


def warp_affine(image, M, dsize, background=0):
    """cv2.warpAffine(image, M, dsize=(width, height), borderMode=BORDER_CONSTANT, borderValue=background) for uint8 images: a NumPy
    (H, W[, C]) image (one upload, one launch, one download) or a `WarpImage` (recorded)."""
    if isinstance(image, (WarpImage, GeoImage, StagedGeoImage, ProgramImage)):
        return image.warp(M, dsize, background)
    if not isinstance(image, np.ndarray):
        raise TypeError("warp_affine takes a NumPy image or a lazy WarpImage / GeoImage")
    if image.dtype != np.uint8:
        raise TypeError("warp_affine takes uint8 images")
    src = image if image.ndim == 3 else image[:, :, None]
    out_w, out_h = int(dsize[0]), int(dsize[1])
    xtab, ytab = warp_tables(M, out_h, out_w)
    geo = np.zeros((1, 5), dtype=np.int32)
    bg = border_value(background, src.shape[2])[None]
    out = nat.image_warp_affine_u8(nat.to_device(np.ascontiguousarray(src)[None]), out_h, out_w, geo, xtab[None], ytab[None], bg)[0].cpu().numpy()
    return out if image.ndim == 3 else out[:, :, 0]
