"""NumPy statement of csrc/ssdhip_evalcollect.hip: what `ssdhip_eval_collect` appends to the device store and what `ssdhip_eval_pack`
builds from it.  tests/test_eval_collect_cpu.py holds it to the Evaluator's host route; tests/test_eval_collect_kernels_gpu.py holds the
kernels to it, bit for bit.

A store is a dict: rows (capacity, 6) of the rows' dtype, image (capacity,) int32, n (rows appended), bad (rows of a class outside
1 .. n_classes or of an image index outside 0 .. n_images - 1), overflow (0 / 1), class_count (n_classes,) -- the kernel's counters."""
import numpy as np

MAX_STEPS, DESC, PACK_CHUNK = 4, 14, 256
SCALE, SHIFT = 0, 1


def new_store(capacity, dtype, n_classes, fill=0.0, guard=0):
    """`guard`: rows allocated behind `capacity` that no append may touch."""
    return {"rows": np.full((capacity + guard, 6), fill, dtype=dtype), "image": np.full((capacity + guard,), -7, dtype=np.int32), "n": 0,
            "bad": 0, "overflow": 0, "class_count": np.zeros((n_classes,), dtype=np.int64), "capacity": capacity}


def make_desc(image_indices, programs):
    """(B, DESC) float64: per image [dataset index, number of steps, (op, a_y, a_x) x MAX_STEPS]."""
    desc = np.zeros((len(image_indices), DESC), dtype=np.float64)
    for b, (index, steps) in enumerate(zip(image_indices, programs)):
        assert len(steps) <= MAX_STEPS
        desc[b, 0], desc[b, 1] = index, len(steps)
        for k, step in enumerate(steps):
            desc[b, 2 + 3 * k:5 + 3 * k] = step
    return desc


def _round(v, decimals):
    """round(v, decimals) of a NumPy scalar, in v's dtype: rint(v * T(10^d)) / T(10^d); 0 leaves the value alone."""
    if not decimals:
        return v
    p = v.dtype.type(10.0 ** decimals)
    return np.rint(v * p) / p


def class_of(v, n_classes):
    """The list `int(box[class_id])` names, 1 .. n_classes; 0 for everything else."""
    return np.where((v >= 1) & (v < n_classes + 1), np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0), 0).astype(np.int64)


def collect(store, rows, count, desc, n_images, n_classes, coord_decimals=1, conf_decimals=0):
    """Append the valid rows of rows (B, R, 6) in (image, row) order.  count (B,) or None (then: class != 0)."""
    B, R = rows.shape[:2]
    T = rows.dtype.type
    valid = [(np.arange(R) < min(max(int(count[b]), 0), R)) if count is not None else (rows[b, :, 0] != 0) for b in range(B)]
    total = int(sum(v.sum() for v in valid))
    if store["n"] + total > store["capacity"]:
        store["overflow"] = 1                                      # an append that does not fit writes nothing at all
        return
    at = store["n"]
    for b in range(B):
        take = rows[b][valid[b]].copy()
        if not take.shape[0]:
            continue
        index = int(desc[b, 0]) if 0 <= desc[b, 0] < n_images else -1
        n_steps = int(desc[b, 1]) if 0 <= desc[b, 1] <= MAX_STEPS else 0
        for k in range(n_steps):
            op, a_y, a_x = desc[b, 2 + 3 * k:5 + 3 * k]
            if op == SCALE:
                take[:, [3, 5]] = np.rint(take[:, [3, 5]] * T(a_y))
                take[:, [2, 4]] = np.rint(take[:, [2, 4]] * T(a_x))
            else:
                take[:, [3, 5]] = take[:, [3, 5]] + T(a_y)
                take[:, [2, 4]] = take[:, [2, 4]] + T(a_x)
        take[:, 1] = _round(take[:, 1], conf_decimals)
        take[:, 2:6] = _round(take[:, 2:6], coord_decimals)
        k = take.shape[0]
        store["rows"][at:at + k] = take
        store["image"][at:at + k] = index
        cls = class_of(take[:, 0], n_classes) if index >= 0 else np.zeros((k,), dtype=np.int64)
        store["bad"] += int((cls == 0).sum())
        store["class_count"] += np.bincount(cls, minlength=n_classes + 1)[1:]
        at += k
    store["n"] = at


def pack(store_rows, store_image, n, n_images, n_classes):
    """Stable counting sort of the first n store rows by class -> pred (P, 5) float32, segment (P,) int32, slot (P,) int32, starts
    (n_classes + 1,) int32; rows of a class outside 1 .. n_classes or an image outside 0 .. n_images - 1 are left out."""
    rows, image = store_rows[:n], store_image[:n].astype(np.int64)
    slot = class_of(rows[:, 0], n_classes) - 1
    slot[(image < 0) | (image >= n_images)] = -1
    keep = np.flatnonzero(slot >= 0)
    order = keep[np.argsort(slot[keep], kind='stable')]
    counts = np.bincount(slot[keep], minlength=n_classes)
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return (rows[order][:, 1:6].astype(np.float32), (slot[order] * n_images + image[order]).astype(np.int32), slot[order].astype(np.int32),
            starts)
