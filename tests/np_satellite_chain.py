"""The walk of csrc/ssdhip_augment.hip's saug_decide_image restated in NumPy: DataAugmentationSatellite's decisions for a batch, draw by
draw on an `np.random.RandomState` -- the photometric programs, the 12-int geometry rows (patched?, top, left, height, width, flipped
horizontally?, vertically?, quarter turns, size in front of the resize x 2, 0, interpolation), the surviving labels and the generator
state(s) -- from the fields of ssdhip_sat_augment_params and the quarter turns drawn in advance.  `walk` is what
`_native.sat_augment_decide` computes; `geometry` states what the plan and gather launches then do with a row, the rotation through
cv2.warpAffine's own arithmetic (tests/np_warp.py) on Rotate's matrix rather than through the index permutation under test."""
import numpy as np

from tests import np_variable_chain as nvc

PROG, MAX_BOXES = nvc.PROG, nvc.MAX_BOXES


def rotate_labels(turns, H, W, x0, y0, x1, y1):
    """Rotate's labels for whole-number coordinates on an H x W image (the closed integer form of the reference's matrix)."""
    if turns == 1:
        return y0, W - x1, y1, W - x0
    if turns == 2:
        return W - x1, H - y1, W - x0, H - y0
    return H - y1, x0, H - y0, x1


def one_image(p, rs, H, W, lab, turns):
    """p: the params dict; lab (n, 5) float64 rows (class_id, xmin, ymin, xmax, ymax); turns: the quarter turns the image takes IF it
    rotates -> (steps, geometry row, surviving rows, rotated?)."""
    steps = [("to_f32", 0.0)]

    def maybe(which, name):
        if rs.uniform(0, 1) >= 1.0 - p["photo_prob"][which]:
            steps.append((name, rs.uniform(p["photo_lower"][which], p["photo_upper"][which])))

    maybe(0, "brightness")
    maybe(1, "contrast")
    steps.extend([("to_u8", 0.0), ("rgb2hsv", 0.0), ("to_f32", 0.0)])
    maybe(2, "saturation")
    maybe(3, "hue")
    steps.extend([("to_u8", 0.0), ("hsv2rgb", 0.0)])

    lab = np.array(lab, dtype=np.float64).reshape(-1, 5)
    n = lab.shape[0]
    alive = np.ones(n, dtype=bool)
    cls, x0, y0, x1, y1 = (lab[:, k].copy() for k in range(5))
    g = [0, 0, 0, H, W, 0, 0, 0, H, W, 0, p["interpolation"]]
    if not (rs.uniform(0, 1) < 1.0 - p["flip_prob"]):
        x0, x1 = W - x1, W - x0
        g[5] = 1
    if not (rs.uniform(0, 1) < 1.0 - p["vflip_prob"]):
        y0, y1 = H - y1, H - y0
        g[6] = 1
    rotated = bool(rs.uniform(0, 1) >= 1.0 - p["rotate_prob"])
    if rotated:
        x0, y0, x1, y1 = rotate_labels(int(turns), float(H), float(W), x0, y0, x1, y1)
        if turns % 2:
            H, W = W, H
        g[7] = int(turns)
    g[3], g[4] = H, W
    crit = p["criterion"]
    if not (rs.uniform(0, 1) < 1.0 - p["patch_prob"]):
        for _ in range(max(1, p["n_trials"])):
            w = int(rs.uniform(p["min_scale"], p["max_scale"]) * W)
            ar = rs.uniform(p["min_aspect_ratio"], p["max_aspect_ratio"])
            h = int(w / ar)
            top = nvc._position(rs, H, h)
            left = nvc._position(rs, W, w)
            sx0, sy0, sx1, sy1 = x0 - left, y0 - top, x1 - left, y1 - top
            n_ok = int(nvc._overlap_ok(crit, sx0, sy0, sx1, sy1, h, w, p["validator_lower"], p["validator_upper"]).sum())
            if (n_ok < p["n_boxes_min"]) if p["n_boxes_min"] > 0 else (n_ok != n):
                continue
            x0, y0, x1, y1 = sx0, sy0, sx1, sy1
            alive &= nvc._overlap_ok(crit, x0, y0, x1, y1, h, w, p["filter_lower"], p["filter_upper"])
            if p["clip_boxes"]:
                y0, y1 = np.clip(y0, 0, h - 1.0), np.clip(y1, 0, h - 1.0)
                x0, x1 = np.clip(x0, 0, w - 1.0), np.clip(x1, 0, w - 1.0)
            g[0:5] = [1, top, left, h, w]
            H, W = h, w
            break
    g[8], g[9] = H, W
    sy, sx = p["out_height"] / H, p["out_width"] / W
    y0, y1, x0, x1 = np.rint(y0 * sy), np.rint(y1 * sy), np.rint(x0 * sx), np.rint(x1 * sx)
    alive &= (x1 > x0) & (y1 > y0) & ((x1 - x0) * (y1 - y0) >= p["resize_min_area"])
    rows = np.stack([cls, x0, y0, x1, y1], axis=1)[alive]
    return steps, np.array(g, dtype=np.int32), rows, rotated


def walk(params, turns, mt_states, labels, n_labels, shapes):
    """mt_states (625,): the batch in order on one state, the k-th image that rotates takes turns[k]; (B, 625): image b on its own state,
    it takes turns[b].  -> (ops (B, 16), args (B, 16), geometry (B, 12), labels_out (B, 64, 5), n_out (B,), mt_states_out)."""
    B = len(shapes)
    stream = np.ndim(mt_states) == 1
    ops, args = np.zeros((B, PROG), dtype=np.int32), np.zeros((B, PROG), dtype=np.float64)
    geo = np.zeros((B, 12), dtype=np.int32)
    lab_out, n_out = np.zeros((B, MAX_BOXES, 5), dtype=np.float64), np.zeros((B,), dtype=np.int32)
    mt_out = np.array(mt_states, dtype=np.uint32)
    rs = nvc.state_of(mt_states) if stream else None
    k = 0
    for b, (H, W) in enumerate(shapes):
        if not stream:
            rs = nvc.state_of(mt_states[b])
        steps, geo[b], rows, rotated = one_image(params, rs, int(H), int(W), labels[b, :int(n_labels[b])], turns[k if stream else b])
        k += int(rotated)
        ops[b], args[b] = nvc.encode(steps)
        n_out[b] = rows.shape[0]
        lab_out[b, :rows.shape[0]] = rows
        if not stream:
            mt_out[b] = nvc.state_row(rs)
    if stream:
        mt_out = nvc.state_row(rs)
    return ops, args, geo, lab_out, n_out, mt_out


def geometry(img, g, out_h, out_w, background):
    """The plan builder and the gather on one image: the flips, the rotation (warpAffine with Rotate's matrix, border 0), the patch window
    (background where it leaves the rotated image), cv2.resize."""
    from oracle import np_image as npi
    from ssd_keras_amd.data_generator import _image_ops as iop
    from tests import np_warp
    if g[5]:
        img = img[:, ::-1]
    if g[6]:
        img = img[::-1]
    if g[7]:
        M, dsize = iop.quarter_turn_matrix(img.shape[0], img.shape[1], 90 * int(g[7]))
        img = np_warp.warp_affine(np.ascontiguousarray(img), M, dsize, 0)
    if g[0]:
        top, left, h, w = (int(v) for v in g[1:5])
        canvas = np.empty((h, w, 3), dtype=np.uint8)
        canvas[:, :] = np.array(background, dtype=np.uint8)
        ya, yb, xa, xb = max(top, 0), min(top + h, img.shape[0]), max(left, 0), min(left + w, img.shape[1])
        if yb > ya and xb > xa:
            canvas[ya - top:yb - top, xa - left:xb - left] = img[ya:yb, xa:xb]
        img = canvas
    return npi.resize(np.ascontiguousarray(img), (out_w, out_h), int(g[11]))


def execute_lazy(im, lazy):
    """A resized GeoImage's index maps executed with NumPy indexing on its (H, W, 3) image: -1 = background, -2 = black, `transposed`
    swaps what the two maps address; then cv2.resize."""
    from oracle import np_image as npi
    return npi.resize(index_maps(im, lazy), (lazy.resized[1], lazy.resized[0]), lazy.resized[2])


def index_maps(im, lazy):
    ys, xs = np.asarray(lazy.ys), np.asarray(lazy.xs)
    a, c = np.clip(ys, 0, None), np.clip(xs, 0, None)
    view = (im[c][:, a].transpose(1, 0, 2) if lazy.transposed else im[a][:, c]).copy()
    black = (ys[:, None] == -2) | (xs[None, :] == -2)
    view[black] = 0
    pad = (ys[:, None] == -1) | (xs[None, :] == -1)
    view[pad] = np.array(lazy.background if lazy.background is not None else (0, 0, 0), dtype=np.uint8)
    return np.ascontiguousarray(view)
