"""The walk of csrc/ssdhip_augment.hip's vaug_decide_image restated in NumPy: DataAugmentationVariableInputSize's decisions for a batch,
draw by draw on an `np.random.RandomState` -- the photometric programs, the 12-int geometry rows, the surviving labels and the generator
state(s) -- from the fields of ssdhip_var_augment_params.  `decide` has the calling convention of `_native.var_augment_decide`, so tests
can put it in that binding's place; `pixels` states what the three pixel launches then do with its outputs."""
import numpy as np

OPS = {"end": 0, "to_f32": 1, "to_u8": 2, "brightness": 3, "contrast": 4, "saturation": 5, "hue": 6, "rgb2hsv": 7, "hsv2rgb": 8}
PROG, MAX_BOXES = 16, 64
CENTER_POINT, IOU, AREA = 0, 1, 2


def state_row(rs):
    st = rs.get_state()
    return np.concatenate([np.asarray(st[1], dtype=np.uint32), np.array([st[2]], dtype=np.uint32)])


def state_of(row):
    rs = np.random.RandomState()
    rs.set_state(('MT19937', np.asarray(row[:624], dtype=np.uint32), int(row[624]), 0, 0.0))
    return rs


def _overlap_ok(criterion, x0, y0, x1, y1, H, W, lower, upper):
    """BoxFilter's overlap test with border_pixels 'half' for float64 vectors of corners against an H x W image."""
    with np.errstate(divide="ignore", invalid="ignore"):
        if criterion == IOU:
            iw = np.maximum(0.0, np.minimum(x1, float(W)) - np.maximum(x0, 0.0))
            ih = np.maximum(0.0, np.minimum(y1, float(H)) - np.maximum(y0, 0.0))
            inter = iw * ih
            union = (float(W) * float(H) + (x1 - x0) * (y1 - y0)) - inter
            v = inter / union
            return (v > lower) & (v <= upper)
        if criterion == AREA:
            box = (x1 - x0) * (y1 - y0)
            cx0, cx1 = np.clip(x0, 0, W - 1.0), np.clip(x1, 0, W - 1.0)
            cy0, cy1 = np.clip(y0, 0, H - 1.0), np.clip(y1, 0, H - 1.0)
            inter = (cx1 - cx0) * (cy1 - cy0)
            return ((inter > lower * box) if lower == 0.0 else (inter >= lower * box)) & (inter <= upper * box)
        cy, cx = (y0 + y1) / 2.0, (x0 + x1) / 2.0
        return (cy >= 0.0) & (cy <= H - 1.0) & (cx >= 0.0) & (cx <= W - 1.0)


def _position(rs, extent, size):
    room = extent - size
    return int(rs.randint(0, room + 1)) if room >= 0 else int(rs.randint(room, 1))


def one_image(p, rs, H, W, lab):
    """p: the params dict; lab (n, 5) float64 rows (class_id, xmin, ymin, xmax, ymax) -> (steps, geometry row, surviving rows, trace)."""
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
    trace = dict(trial=0, patch_dropped=0, resize_dropped=0)
    crit = p["criterion"]
    if not (rs.uniform(0, 1) < 1.0 - p["patch_prob"]):
        for t in range(max(1, p["n_trials"])):
            w = int(rs.uniform(p["min_scale"], p["max_scale"]) * W)
            ar = rs.uniform(p["min_aspect_ratio"], p["max_aspect_ratio"])
            h = int(w / ar)
            top = _position(rs, H, h)
            left = _position(rs, W, w)
            sx0, sy0, sx1, sy1 = x0 - left, y0 - top, x1 - left, y1 - top
            n_ok = int(_overlap_ok(crit, sx0, sy0, sx1, sy1, h, w, p["validator_lower"], p["validator_upper"]).sum())
            if (n_ok < p["n_boxes_min"]) if p["n_boxes_min"] > 0 else (n_ok != n):
                continue
            x0, y0, x1, y1 = sx0, sy0, sx1, sy1
            keep = _overlap_ok(crit, x0, y0, x1, y1, h, w, p["filter_lower"], p["filter_upper"])
            trace["patch_dropped"] = int((~keep).sum())
            alive &= keep
            if p["clip_boxes"]:
                y0, y1 = np.clip(y0, 0, h - 1.0), np.clip(y1, 0, h - 1.0)
                x0, x1 = np.clip(x0, 0, w - 1.0), np.clip(x1, 0, w - 1.0)
            g[0:5] = [1, top, left, h, w]
            trace["trial"] = t + 1
            H, W = h, w
            break
    g[8], g[9] = H, W
    if not (rs.uniform(0, 1) < 1.0 - p["flip_prob"]):
        x0, x1 = W - x1, W - x0
        g[10] = 1
    sy, sx = p["out_height"] / H, p["out_width"] / W
    y0, y1, x0, x1 = np.rint(y0 * sy), np.rint(y1 * sy), np.rint(x0 * sx), np.rint(x1 * sx)
    big = (x1 > x0) & (y1 > y0) & ((x1 - x0) * (y1 - y0) >= p["resize_min_area"])
    trace["resize_dropped"] = int((alive & ~big).sum())
    alive &= big
    rows = np.stack([cls, x0, y0, x1, y1], axis=1)[alive]
    return steps, np.array(g, dtype=np.int32), rows, trace


def encode(steps):
    ops, args = np.zeros(PROG, dtype=np.int32), np.zeros(PROG, dtype=np.float64)
    for k, (name, arg) in enumerate(steps):
        ops[k], args[k] = OPS[name], arg
    return ops, args


def walk(params, mt_states, labels, n_labels, shapes):
    """mt_states (625,): the batch in order on one state; (B, 625): image b on its own.  labels (B, 64, 5) float64, n_labels (B,).
    -> (ops (B, 16), args (B, 16), geometry (B, 12), labels_out (B, 64, 5), n_out (B,), mt_states_out, traces)."""
    B = len(shapes)
    stream = np.ndim(mt_states) == 1
    ops, args = np.zeros((B, PROG), dtype=np.int32), np.zeros((B, PROG), dtype=np.float64)
    geo = np.zeros((B, 12), dtype=np.int32)
    lab_out, n_out = np.zeros((B, MAX_BOXES, 5), dtype=np.float64), np.zeros((B,), dtype=np.int32)
    mt_out = np.array(mt_states, dtype=np.uint32)
    rs = state_of(mt_states) if stream else None
    traces = []
    for b, (H, W) in enumerate(shapes):
        if not stream:
            rs = state_of(mt_states[b])
        steps, geo[b], rows, trace = one_image(params, rs, int(H), int(W), labels[b, :int(n_labels[b])])
        ops[b], args[b] = encode(steps)
        n_out[b] = rows.shape[0]
        lab_out[b, :rows.shape[0]] = rows
        traces.append(trace)
        if not stream:
            mt_out[b] = state_row(rs)
    if stream:
        mt_out = state_row(rs)
    return ops, args, geo, lab_out, n_out, mt_out, traces


def pixels(image, ops, args, g, out_h, out_w, background):
    """What the three pixel launches make of one (H, W, 3) uint8 image: its program, then `geometry` -- oracle/np_image.py's statements
    of those kernels."""
    from oracle import np_image as npi
    return geometry(npi.run_program(image, ops, args), g, out_h, out_w, background)


def geometry(img, g, out_h, out_w, background):
    """The plan builder and the gather on one image: the patch window (background where it leaves the image), the flip, cv2.resize."""
    from oracle import np_image as npi
    if g[0]:
        top, left, h, w = (int(v) for v in g[1:5])
        canvas = np.empty((h, w, 3), dtype=np.uint8)
        canvas[:, :] = np.array(background, dtype=np.uint8)
        ya, yb, xa, xb = max(top, 0), min(top + h, img.shape[0]), max(left, 0), min(left + w, img.shape[1])
        if yb > ya and xb > xa:
            canvas[ya - top:yb - top, xa - left:xb - left] = img[ya:yb, xa:xb]
        img = canvas
    if g[10]:
        img = img[:, ::-1]
    return npi.resize(np.ascontiguousarray(img), (out_w, out_h), int(g[11]))
