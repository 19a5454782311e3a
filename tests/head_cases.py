"""Case tables and data builders of tests/test_head_assembly_gpu.py and tests/test_decode_from_heads_gpu.py: the prediction assembly
(csrc/ssdhip_heads.h, head_build_rows) through each of its four source paths -- float32 packed heads, packed bf16 by LDS-DMA, dense
bf16 spans, packed bf16 by the element-wise gather -- at the smallest maps that reach each seam of its tiling.

Every case carries its plan: the tile size TA, the tiles and the anchors of the last tile of every layer, the number of tile
boundaries that fall inside a pixel, and the source path of every layer.  `plan_of` recomputes it from the library's export
(`ssdhip_head_tile_anchors`: host arithmetic, no launch) and from the host-decidable conditions of the LDS-DMA path, and
tests/test_head_reference_cpu.py asserts it for every case, so a change of the tile sizes or of the path conditions that moves a case
off its seam fails without a GPU.

A layer is (h, w, n_boxes, form, conf bias?, loc bias?).  Forms:
  dense    two arrays, conf [B, h, w, n_boxes C] and loc [B, h, w, n_boxes 4]
  dma      one packed array [conf | loc | padding], channels rounded up to a multiple of 64 (what the models' head convolutions write)
  dma8     ... rounded up to the smallest multiple of 8
  tight    ... exactly n_boxes (C + 4) channels: the gather wherever that is no multiple of 8
  offbase  dma8's array viewed 4 elements (8 bytes) behind a 16-byte boundary of a larger flat buffer: the gather
  f32      float32 packed array (bias already inside), channels rounded up to a multiple of 8;  f32t: exactly n_boxes (C + 4)
Padding channels hold NaN in every packed form.

Data conditions (asserted by the CPU test for every case): bf16 head outputs and biases are multiples of 2^-6 below 16 in magnitude,
so conf + bias is exact in float32 and in float64 and its one rounding to bf16 is the only rounding (ties occur: the sums have up to
11 significant bits); |logit| <= 16 after the bias; everything finite; float32 heads hold float32 numbers with |logit| <= 16.

The 2 GB source guard of the LDS-DMA path (src_bytes < 0x7fffff00) cannot be reached at test sizes: no case fails it."""
import zlib

import numpy as np

from tests import np_heads as ref

MAX_LAYERS = 8                                            # csrc/ssdhip_heads.h: MAX_PRED_LAYERS


def _rng(*key):
    return np.random.RandomState(zlib.crc32(repr(key).encode()))


# ---- the library's tile arithmetic ------------------------------------------------------------------------------------------------
def _lib():
    from ssd_keras_amd import _native as nat
    return nat.load()


def tile_anchors(C, for_decode=False):
    return int(_lib().ssdhip_head_tile_anchors(int(C), int(bool(for_decode))))


def tile_steps(for_decode=False, upto=1100):
    """[(C, TA)] wherever TA changes as C grows from 2: [(2, 256), (27, 128), ...]; TA 0 = refused."""
    steps, last = [], None
    for C in range(2, upto):
        ta = tile_anchors(C, for_decode)
        if ta != last:
            steps.append((C, ta))
            last = ta
    return steps


# As derived from head_tile_lds = TA (6 C + 72) + 64 C + 1280 bytes against 60 KB (tiles) and 64 KB (a launch), and reported by the export.
ASSEMBLY_STEPS = [(2, 256), (27, 128), (62, 64), (125, 32), (243, 0)]
DECODE_STEPS = [(2, 256), (27, 128), (62, 64), (125, 0)]


def stage_bytes(TA, C):
    """csrc/ssdhip_heads.h, head_stage_bytes."""
    return TA * (C + 4) * 2 + 16 * TA + 64 * (C + 4) + 1024


def stride_of(form, nb, C):
    need = nb * (C + 4)
    if form == "dense":
        return None
    if form == "dma":
        return -(-need // 64) * 64
    if form in ("dma8", "offbase", "f32"):
        return -(-need // 8) * 8
    assert form in ("tight", "f32t"), form
    return need


def staging_fits(TA, C, nb, n_anchors):
    """The staging-size condition of the LDS-DMA path for every tile of a layer: the tile's pixel rows as 16-byte chunks in whole
    1 KB pieces, plus the biases, within head_stage_bytes."""
    U = nb * (C + 4) * 2
    cpr = (U + 15) // 16
    for a0 in range(0, n_anchors, TA):
        na = min(TA, n_anchors - a0)
        npx = (a0 + na - 1) // nb - a0 // nb + 1
        if ((npx * cpr + 63) // 64) * 1024 + U > stage_bytes(TA, C):
            return False
    return True


def source_path(form, TA, C, nb, n_anchors, dma_enabled=True):
    """'F' float32, 'L' LDS-DMA, 'D' dense spans, 'G' gather: which branch of head_build_rows a layer takes, from what the host can
    see (stride, base alignment, SSDHIP_HEADS_DMA, the staging size; head_kernel and scan_heads_kernel run whole waves)."""
    if form in ("f32", "f32t"):
        return "F"
    if form == "dense":
        return "D"                                     # (a dense pair never has loc behind conf at one stride)
    stride = stride_of(form, nb, C)
    pitch = (nb * (C + 4) * 2 + 15) // 16 * 16
    if dma_enabled and form != "offbase" and stride % 8 == 0 and stride * 2 >= pitch and staging_fits(TA, C, nb, n_anchors):
        return "L"
    return "G"


def plan_of(C, layers, TA, dma_enabled=True):
    tiles, last, mid, paths = [], [], 0, []
    for h, w, nb, form, _, _ in layers:
        na = h * w * nb
        t = -(-na // TA)
        tiles.append(t)
        last.append(na - (t - 1) * TA)
        mid += sum(1 for k in range(1, t) if (k * TA) % nb)
        paths.append(source_path(form, TA, C, nb, na, dma_enabled))
    return TA, tuple(tiles), tuple(last), mid, "".join(paths)


# ---- cases ------------------------------------------------------------------------------------------------------------------------
# name -> (C, B, anchors_var off a 16-byte boundary?, layers, plan = (TA, tiles, anchors of the last tile, boundaries inside a pixel, paths))
T, F = True, False
CASES = {
    # 256-anchor tiles.  21 classes: every form in one launch; 3 and 5 boxes put a tile boundary inside a pixel and leave a partial tile
    "c21_mixed": (21, 3, F, [(9, 10, 3, "dma", T, T), (4, 13, 5, "tight", T, F), (8, 8, 4, "dense", F, T), (1, 1, 6, "dma8", F, F),
                             (1, 1, 1, "offbase", T, T), (3, 5, 8, "dma", T, T)],
                  (256, (2, 2, 1, 1, 1, 1), (14, 4, 256, 6, 1, 120), 2, "LGDLGL")),
    # the last class count of the 256-anchor tile; anchors_var off alignment (the DMA path's scalar anchor copy)
    "c26_last256": (26, 1, T, [(1, 43, 6, "tight", T, T), (7, 13, 3, "dma8", T, T), (2, 2, 4, "dense", T, T)],
                    (256, (2, 2, 1), (2, 17, 16), 2, "GLD")),
    "c2_smallest": (2, 3, F, [(2, 43, 3, "tight", T, T), (4, 13, 5, "dma8", F, T), (16, 16, 1, "dense", T, F), (1, 1, 8, "dma", T, T)],
                    (256, (2, 2, 1, 1), (2, 4, 256, 8), 2, "GLDL")),
    "c6_offbase": (6, 1, T, [(3, 29, 3, "offbase", T, T), (1, 1, 1, "tight", T, T), (5, 11, 5, "dense", T, T), (5, 13, 4, "dma8", F, F)],
                   (256, (2, 1, 2, 2), (5, 1, 19, 4), 2, "GGDL")),
    # 128-anchor tiles: the first and the last class count
    "c27_first128": (27, 3, F, [(5, 9, 3, "dma", T, T), (1, 16, 8, "dma8", T, F), (3, 9, 5, "tight", F, T), (1, 1, 4, "offbase", T, T)],
                     (128, (2, 1, 2, 1), (7, 128, 7, 4), 2, "LLGG")),
    "c61_last128": (61, 1, F, [(1, 26, 5, "tight", T, T), (4, 11, 3, "dma8", T, T), (2, 16, 4, "dense", T, T), (3, 29, 3, "dma", F, F)],
                    (128, (2, 2, 1, 3), (2, 4, 128, 5), 4, "GLDL")),
    # a geometry that fails ONLY the staging-size condition of the LDS-DMA path (aligned base, stride a multiple of 8, DMA enabled):
    # 36 boxes of 65 values are 293 16-byte chunks per pixel; the first tile touches 4 pixels = 19 456 bytes of chunks + 4 680 of biases
    # against 23 872 of staging.  Such box counts (14 and up, by host arithmetic over every C and tile) take the gather.
    "c61_staging": (61, 1, F, [(1, 4, 36, "dma8", T, T), (1, 2, 3, "dma8", T, T)], (128, (2, 1), (16, 6), 1, "GL")),
    # 64-anchor tiles
    "c62_first64": (62, 3, T, [(1, 22, 3, "tight", T, T), (2, 7, 5, "dma8", T, T), (4, 4, 4, "dense", F, F), (1, 1, 8, "dma", T, F)],
                    (64, (2, 2, 1, 1), (2, 6, 64, 8), 2, "GLDL")),
    "c81_coco": (81, 1, F, [(3, 5, 6, "dma", T, T), (1, 13, 5, "tight", T, T), (1, 8, 8, "offbase", F, T), (1, 1, 3, "dense", T, T)],
                 (64, (2, 2, 1, 1), (26, 1, 64, 3), 2, "LGGD")),
    "c124_last64": (124, 1, F, [(1, 22, 3, "dma8", T, T), (1, 13, 5, "offbase", T, T), (2, 8, 4, "dense", T, T), (1, 1, 1, "tight", T, T)],
                    (64, (2, 2, 1, 1), (2, 1, 64, 1), 2, "LGDL")),
    # 32-anchor tiles: the assembly only (decode from heads refuses them); the first and the last class count a launch takes
    "c125_first32": (125, 1, F, [(1, 11, 3, "dma8", T, T), (1, 7, 5, "tight", T, T), (1, 4, 8, "dense", T, T), (1, 1, 6, "dma", F, T)],
                     (32, (2, 2, 1, 1), (1, 3, 32, 6), 2, "LGDL")),
    "c242_last": (242, 1, T, [(1, 11, 3, "tight", T, T), (2, 4, 4, "dma8", T, T), (1, 7, 5, "dense", T, F)],
                  (32, (2, 1, 2), (1, 32, 3), 2, "GLD")),
    # the eight layers the ABI takes, every box count, every form
    "c21_eight": (21, 3, F, [(2, 3, 1, "dma8", T, T), (3, 3, 3, "tight", T, T), (2, 2, 4, "dense", T, T), (1, 2, 5, "offbase", T, T),
                             (1, 1, 6, "dma", F, F), (4, 9, 8, "dma", T, T), (1, 3, 4, "tight", T, T), (2, 1, 6, "dense", F, T)],
                  (256, (1, 1, 1, 1, 1, 2, 1, 1), (6, 27, 16, 10, 6, 32, 12, 12), 0, "LGDGLLGD")),
    # float32 packed heads (models/precise.py): one per tile size
    "f32_c21": (21, 3, F, [(9, 10, 3, "f32", F, F), (4, 13, 5, "f32t", F, F), (8, 8, 4, "f32", F, F), (1, 1, 6, "f32t", F, F)],
                (256, (2, 2, 1, 1), (14, 4, 256, 6), 2, "FFFF")),
    "f32_c27": (27, 1, T, [(5, 9, 3, "f32t", F, F), (1, 16, 8, "f32", F, F), (1, 1, 1, "f32t", F, F)],
                (128, (2, 1, 1), (7, 128, 1), 1, "FFF")),
    "f32_c81": (81, 3, F, [(1, 13, 5, "f32t", F, F), (3, 5, 6, "f32", F, F), (2, 8, 4, "f32", F, F)],
                (64, (2, 2, 1), (1, 26, 64), 2, "FFF")),
    "f32_c125": (125, 1, F, [(1, 11, 3, "f32t", F, F), (1, 4, 8, "f32", F, F), (1, 7, 5, "f32", F, F)],
                 (32, (2, 1, 2), (1, 32, 3), 2, "FFF")),
}
BF16_CASES = [n for n in CASES if not n.startswith("f32")]
F32_CASES = [n for n in CASES if n.startswith("f32")]
# the cases decode-from-heads runs (every TA form it has, all four paths): path equality and planted detections
DECODE_CASES = ["c21_mixed", "c27_first128", "c62_first64", "c81_coco", "f32_c21", "f32_c27", "f32_c81"]
# backward of the assembly: (C, B, [(h, w, n_boxes, packed channels: "8" = the smallest multiple of 8, "128" = of 128)]).  head_grad_kernel
# tiles 128 / n_boxes whole pixels; its row tiles start at float (b N + first anchor of the tile) (C + 12) of y_pred: with C + 12 odd
# (C = 21, 27) the anchors 0, 1, 2, 3 mod 4 give all four residues mod 4 of that start, with C + 12 = 2 mod 4 (C = 2, 26, 62) two of
# them, with C + 12 a multiple of 4 (C = 36) one.  `residues` is asserted by the CPU test.
BACKWARD_CASES = {
    "bwd_c21": (21, 3, [(1, 1, 1, "8"), (6, 9, 3, "8"), (2, 3, 5, "128"), (3, 7, 8, "8"), (7, 5, 4, "128"), (1, 1, 6, "8")], (0, 1, 2, 3)),
    "bwd_c27": (27, 1, [(9, 15, 1, "8"), (1, 1, 3, "128"), (9, 3, 5, "8"), (1, 17, 8, "128")], (0, 1, 2, 3)),
    "bwd_c26": (26, 3, [(1, 1, 5, "8"), (5, 9, 3, "128"), (1, 1, 1, "8"), (2, 9, 8, "8")], (0, 2)),
    "bwd_c36": (36, 1, [(3, 15, 3, "8"), (1, 1, 8, "128"), (2, 13, 5, "8"), (3, 43, 1, "8")], (0,)),
    "bwd_c2": (2, 3, [(1, 1, 3, "8"), (3, 43, 1, "128"), (1, 27, 5, "8"), (2, 9, 8, "8")], (0, 2)),
    "bwd_c81": (81, 1, [(1, 1, 1, "8"), (1, 43, 3, "8"), (1, 17, 8, "128"), (2, 13, 5, "8")], (0, 1, 2, 3)),
}
HG_TILE = 128                                             # csrc/ssdhip_layers.hip


def backward_geometry(name):
    """(C, B, maps [(h, w)], n_boxes, strides, the float offsets of every tile's start in y_pred)."""
    C, B, layers, _ = BACKWARD_CASES[name]
    maps = [(h, w) for h, w, _, _ in layers]
    nbs = [nb for _, _, nb, _ in layers]
    strides = [-(-(nb * (C + 4)) // int(m)) * int(m) for _, _, nb, m in layers]
    N = sum(h * w * nb for h, w, nb, _ in layers)
    starts, off = [], 0
    for (h, w), nb in zip(maps, nbs):
        ta = HG_TILE // nb * nb
        for b in range(B):
            starts += [(b * N + off + a0) * (C + 12) for a0 in range(0, h * w * nb, ta)]
        off += h * w * nb
    return C, B, maps, nbs, strides, starts


def case_geometry(name):
    C, B, av_off, layers, plan = CASES[name]
    N = sum(h * w * nb for h, w, nb, _, _, _ in layers)
    return C, B, av_off, layers, plan, N


# ---- data -------------------------------------------------------------------------------------------------------------------------
def _grid(rng, shape, scale, lim):
    """Multiples of 2^-6 within +-lim that are bf16 numbers."""
    return ref.bf16_round(np.clip(np.rint(rng.standard_normal(shape) * scale * 64) / 64, -lim, lim))


def case_data(name):
    """The case's logits, offsets, biases and anchors as float64 arrays, whatever the form they are presented in:
    dict(conf=[B, h, w, nb C], loc=[B, h, w, nb 4], cb=[nb C] or None, lb=[nb 4] or None) per layer, anchors_var [N, 8]."""
    C, B, av_off, layers, plan, N = case_geometry(name)
    rng = _rng("heads", name)
    f32 = name.startswith("f32")
    out = []
    for h, w, nb, form, has_cb, has_lb in layers:
        if f32:
            conf = np.clip(rng.standard_normal((B, h, w, nb * C)) * 3, -16, 16).astype(np.float32).astype(np.float64)
            loc = (rng.standard_normal((B, h, w, nb * 4)) * 2).astype(np.float32).astype(np.float64)
        else:
            conf = _grid(rng, (B, h, w, nb * C), 3.0, 11.0)
            loc = _grid(rng, (B, h, w, nb * 4), 2.0, 11.0)
        cb = _grid(rng, (nb * C,), 1.5, 4.0) if has_cb else None
        lb = _grid(rng, (nb * 4,), 1.5, 4.0) if has_lb else None
        out.append(dict(conf=conf, loc=loc, cb=cb, lb=lb))
    av = rng.random_sample((N, 8)).astype(np.float32).astype(np.float64)
    return out, av


def reference(name, data=None, av=None):
    C, B, av_off, layers, plan, N = case_geometry(name)
    if data is None:
        data, av = case_data(name)
    nbs = [l[2] for l in layers]
    return ref.assemble([d["conf"] for d in data], [d["loc"] for d in data], [d["cb"] for d in data], [d["lb"] for d in data],
                        nbs, av, C, src="f32" if name.startswith("f32") else "bf16")


def packed_array(conf, loc, stride, fill=np.nan):
    """[conf | loc | padding filled with `fill`]: [B, h, w, stride]."""
    b, h, w, _ = conf.shape
    out = np.full((b, h, w, stride), fill, dtype=np.float64)
    out[..., :conf.shape[3]] = conf
    out[..., conf.shape[3]:conf.shape[3] + loc.shape[3]] = loc
    return out


def device_heads(torch, C, layers, data, forms=None):
    """The arguments of nat.assemble_predictions / nat.decode_from_heads for `data` presented in each layer's form (or in `forms`):
    (confs, locs, conf biases, loc biases, n_boxes) -- (B, channels, h, w) views of NHWC memory on the GPU."""
    confs, locs, cbs, lbs = [], [], [], []
    for i, ((h, w, nb, form, _, _), d) in enumerate(zip(layers, data)):
        form = forms[i] if forms is not None else form
        dt = torch.float32 if form in ("f32", "f32t") else torch.bfloat16
        if form == "dense":
            confs.append(torch.from_numpy(d["conf"]).to(dt).cuda().permute(0, 3, 1, 2))
            locs.append(torch.from_numpy(d["loc"]).to(dt).cuda().permute(0, 3, 1, 2))
        else:
            arr = torch.from_numpy(packed_array(d["conf"], d["loc"], stride_of(form, nb, C))).to(dt)
            if form == "offbase":                          # 4 elements behind a 16-byte boundary of a larger flat buffer
                flat = torch.full((arr.numel() + 16,), float("nan"), dtype=dt, device="cuda")
                assert flat.data_ptr() % 16 == 0
                flat[4:4 + arr.numel()] = arr.reshape(-1).cuda()
                t = flat[4:4 + arr.numel()].view(arr.shape)
                assert t.data_ptr() % 16 == 8
            else:
                t = arr.cuda()
                assert t.data_ptr() % 16 == 0
            confs.append(t.permute(0, 3, 1, 2))
            locs.append(None)
        cbs.append(torch.from_numpy(d["cb"]).to(torch.bfloat16).cuda() if d["cb"] is not None else None)
        lbs.append(torch.from_numpy(d["lb"]).to(torch.bfloat16).cuda() if d["lb"] is not None else None)
    return confs, locs, cbs, lbs, [l[2] for l in layers]


def device_anchors(torch, av, off):
    """anchors_var on the GPU; `off`: 4 bytes behind a 16-byte boundary (the scalar anchor copy of the LDS-DMA path)."""
    n = av.shape[0]
    buf = torch.zeros((n * 8 + 4,), dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0
    t = buf[1:1 + n * 8] if off else buf[:n * 8]
    t.copy_(torch.from_numpy(av.astype(np.float32)).reshape(-1))
    t = t.view(n, 8)
    assert t.data_ptr() % 16 == (4 if off else 0)
    return t


# ---- planted detections (tests/test_decode_from_heads_gpu.py)----------------------------------------------------------------------
PLANT_LOGITS = [2.0 + 0.125 * k for k in range(49)]       # distinct bf16 numbers in [2, 8]: neighbouring confidences differ by > 4e-5
GRID = 64                                                 # anchors sit in the cells of a GRID x GRID raster of the unit square


def planted_anchors(N):
    """anchors_var [N, 8]: anchor i is the centroid box of cell i of the raster, half a cell wide and high (pairwise disjoint, every
    coordinate a dyadic number: the corner form and its product with 300 are exact in float32), variances 0.1, 0.1, 0.2, 0.2."""
    assert N <= GRID * GRID
    i = np.arange(N)
    av = np.empty((N, 8))
    av[:, 0] = (i % GRID + 0.5) / GRID
    av[:, 1] = (i // GRID + 0.5) / GRID
    av[:, 2] = av[:, 3] = 0.5 / GRID
    av[:, 4:] = [0.1, 0.1, 0.2, 0.2]
    return av.astype(np.float32).astype(np.float64)


def plant_sites(layers, TA):
    """Global anchor indices at the seams: first and last anchor of every tile (so: of every layer, the last anchor of a layer and the
    first of the next, box n_boxes - 1 of a layer's last pixel), and the middle anchor of every partial last tile."""
    sites, off = [], 0
    for h, w, nb, *_ in layers:
        na = h * w * nb
        for a0 in range(0, na, TA):
            n = min(TA, na - a0)
            sites += [off + a0, off + a0 + n - 1]
            if n < TA and a0 > 0:
                sites.append(off + a0 + n // 2)
        off += na
    return sorted(set(sites))


def planted(name):
    """[(image, global anchor, class, logit)]: image b of B > 1 leaves out every B-th site (a different one in each image); classes
    cycle through 1, C - 1 and the ones between; logits distinct within an image."""
    C, B, av_off, layers, plan, N = case_geometry(name)
    sites = plant_sites(layers, plan[0])
    classes = [1, C - 1] + list(range(2, C - 1))
    out = []
    for b in range(B):
        mine = [s for k, s in enumerate(sites) if B == 1 or (k + b) % B]
        assert len(mine) <= len(PLANT_LOGITS)
        for k, s in enumerate(mine):
            out.append((b, s, classes[(k + b) % len(classes)], PLANT_LOGITS[(5 * k + 3 * b) % len(PLANT_LOGITS)]))
    return out


def planted_data(name):
    """The head outputs of the planted case (no biases, offsets zero): background logit 8 and zeros everywhere, at a planted anchor
    the planted class's logit and zeros."""
    C, B, av_off, layers, plan, N = case_geometry(name)
    z = np.zeros((B, N, C))
    z[:, :, 0] = 8.0
    for b, a, c, s in planted(name):
        z[b, a, :] = 0.0
        z[b, a, c] = s
    data, off = [], 0
    for h, w, nb, *_ in layers:
        n = h * w * nb
        data.append(dict(conf=z[:, off:off + n].reshape(B, h, w, nb * C), loc=np.zeros((B, h, w, nb * 4)), cb=None, lb=None))
        off += n
    return data, planted_anchors(N)


def planted_threshold(C):
    """Between the largest confidence that must stay out -- another class of a planted anchor, 1 / (e^2 + C - 1) -- and the smallest
    planted one, e^2 / (e^2 + C - 1)."""
    return float(np.e / (np.e ** 2 + C - 1))


def planted_expected(name, img_size):
    """Per image the rows [class, confidence, xmin, ymin, xmax, ymax] (float64) and the anchor indices, ordered by confidence."""
    C, B, av_off, layers, plan, N = case_geometry(name)
    av = planted_anchors(N)
    rows = [[] for _ in range(B)]
    for b, a, c, s in planted(name):
        conf = np.exp(s) / (np.exp(s) + (C - 1))
        cx, cy, w, h = av[a, :4]
        rows[b].append((conf, a, [c, conf, (cx - 0.5 * w) * img_size, (cy - 0.5 * h) * img_size, (cx + 0.5 * w) * img_size,
                                  (cy + 0.5 * h) * img_size]))
    out = []
    for r in rows:
        r.sort(key=lambda t: -t[0])
        out.append((np.array([t[2] for t in r]), np.array([t[1] for t in r])))
    return out
