"""The DataGenerator fixtures and the calls whose results tests/golden/make_data_generator_golden.py records from the reference.

`write_fixtures()` writes small images of different sizes (one grey, one RGBA), four images of one size, a CSV and a COCO-style JSON
annotation file under tests/golden/data_generator/.  `run_reference(ns)` / `run_generate(ns, ...)` call a DataGenerator (the reference's
or the package's, through the namespace `ns`) and return flat dicts of NumPy arrays, so both sides are compared key by key."""
import csv
import json
import os
import warnings

import numpy as np

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data_generator")
# (name, shape): 2-D = grey ('L'), 4 channels = RGBA
IMAGES = [("img_a.png", (37, 53, 3)), ("img_b.png", (48, 40, 3)), ("img_c.png", (29, 61)), ("img_d.png", (44, 44, 4)),
          ("img_e.png", (52, 35, 3)), ("img_f.png", (33, 47, 3)), ("img_g.png", (41, 58, 3)), ("img_h.png", (60, 39, 3))]
EQUAL = [("eq_%d.png" % i, (18, 22, 3)) for i in range(4)]
CSV_FORMAT = ['image_name', 'xmin', 'xmax', 'ymin', 'ymax', 'class_id']
PREDICTIONS = np.array([[1, 0.9, 10, 20, 150, 200], [2, 0.5, 0, 0, 299, 299], [3, 0.25, 100.4, 37.6, 101.5, 38.5]], dtype=np.float64)


def _image(rng, shape):
    """Smooth content (gradients + a few flat rectangles): compresses well and exercises every interpolation."""
    h, w = shape[:2]
    c = shape[2] if len(shape) == 3 else 1
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    planes = []
    for k in range(c):
        a, b, o = rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(40, 200)
        planes.append(o + a * yy + b * xx)
    img = np.stack(planes, axis=-1)
    for _ in range(3):
        y0, x0 = rng.randint(0, h - 4), rng.randint(0, w - 4)
        img[y0:y0 + rng.randint(3, h // 2), x0:x0 + rng.randint(3, w // 2)] = rng.randint(0, 256, size=c)
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return img[:, :, 0] if len(shape) == 2 else img


def _boxes(rng, h, w, n):
    rows = []
    for _ in range(n):
        x0, y0 = rng.randint(0, w - 8), rng.randint(0, h - 8)
        rows.append([int(rng.randint(1, 4)), x0, y0, int(rng.randint(x0 + 4, w)), int(rng.randint(y0 + 4, h))])
    return rows


def write_fixtures():
    from PIL import Image
    os.makedirs(FIXTURES, exist_ok=True)
    rng = np.random.RandomState(2024)
    rows, coco_images, coco_annotations = [], [], []
    for k, (name, shape) in enumerate(IMAGES):
        img = _image(rng, shape)
        Image.fromarray(img, mode={2: 'L', 3: 'RGB', 4: 'RGBA'}[img.ndim if img.ndim == 2 else img.shape[2]]).save(os.path.join(FIXTURES, name))
        boxes = _boxes(rng, shape[0], shape[1], 1 + k % 3)
        for cls, x0, y0, x1, y1 in boxes:
            rows.append([name, x0, x1, y0, y1, cls])
        coco_images.append({"id": 100 + 7 * k, "file_name": name, "height": shape[0], "width": shape[1]})
        for cls, x0, y0, x1, y1 in boxes:
            coco_annotations.append({"id": len(coco_annotations) + 1, "image_id": 100 + 7 * k, "category_id": [1, 3, 7][cls - 1],
                                     "bbox": [x0 + 0.5, y0 + 0.25, float(x1 - x0), float(y1 - y0)]})
    for name, shape in EQUAL:
        Image.fromarray(_image(rng, shape)).save(os.path.join(FIXTURES, name))
    with open(os.path.join(FIXTURES, "labels.csv"), "w", newline='') as f:
        wr = csv.writer(f)
        wr.writerow(CSV_FORMAT)
        wr.writerows(rows)
    coco = {"images": coco_images, "annotations": coco_annotations,
            "categories": [{"id": 1, "name": "one"}, {"id": 3, "name": "three"}, {"id": 7, "name": "seven"}]}
    with open(os.path.join(FIXTURES, "annotations.json"), "w") as f:
        json.dump(coco, f, indent=0, sort_keys=True)


def _state(out, key):
    st = np.random.get_state()
    out[key] = np.concatenate([st[1].astype(np.int64), [int(st[2])]])


def _labels(out, key, labels):
    arrs = [np.asarray(a, dtype=np.float64).reshape(-1, 5) for a in labels]
    out[key + "_n"] = np.array([a.shape[0] for a in arrs], dtype=np.int64)
    out[key] = np.concatenate(arrs) if arrs else np.zeros((0, 5))


def csv_generator(ns, **kw):
    g = ns.DataGenerator(**kw)
    g.parse_csv(images_dir=FIXTURES, labels_filename=os.path.join(FIXTURES, "labels.csv"), input_format=CSV_FORMAT, verbose=False)
    return g


def record_parsers(ns, out):
    g = csv_generator(ns)
    out["csv_filenames"] = np.array([os.path.basename(f) for f in g.filenames])
    out["csv_ids"] = np.array(g.image_ids)
    _labels(out, "csv_labels", g.labels)
    j = ns.DataGenerator()
    j.parse_json(images_dirs=[FIXTURES], annotations_filenames=[os.path.join(FIXTURES, "annotations.json")], ground_truth_available=True,
                 verbose=False)
    out["json_filenames"] = np.array([os.path.basename(f) for f in j.filenames])
    out["json_ids"] = np.array(j.image_ids)
    _labels(out, "json_labels", j.labels)
    out["json_cats_to_classes"] = np.array(sorted(j.cats_to_classes.items()))
    out["json_classes_to_names"] = np.array(j.classes_to_names)


def record_batches(out, tag, gen, returns, n_batches):
    """next(gen) n_batches times; every return recorded (images, labels, ids, inverters applied to PREDICTIONS) + the np.random state."""
    order = ['processed_images', 'encoded_labels', 'matched_anchors', 'processed_labels', 'filenames', 'image_ids', 'evaluation-neutral',
             'inverse_transform', 'original_images', 'original_labels']
    for b in range(n_batches):
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            got = next(gen)
        out["%s_b%d_warnings" % (tag, b)] = np.array([str(w.message) for w in caught] or [""])
        named = dict(zip([r for r in order if r in returns], got))
        key = "%s_b%d_" % (tag, b)
        if 'processed_images' in named:
            out[key + "images"] = np.asarray(named['processed_images'])
        for r in ('processed_labels', 'original_labels'):
            if r in named:
                _labels(out, key + r, named[r])
        if 'image_ids' in named:
            out[key + "ids"] = np.array(named['image_ids'])
        if 'filenames' in named:
            out[key + "filenames"] = np.array([os.path.basename(f) for f in named['filenames']])
        if 'evaluation-neutral' in named:
            out[key + "neutral"] = np.array([len(v) for v in named['evaluation-neutral']] if named['evaluation-neutral'] is not None else [-1])
        if 'inverse_transform' in named:
            inv = []
            for inverters in named['inverse_transform']:
                p = np.copy(PREDICTIONS)
                for f in inverters:
                    p = f(p)
                inv.append(p)
            out[key + "inverted"] = np.stack(inv) if inv else np.zeros((0,) + PREDICTIONS.shape)
            out[key + "n_inverters"] = np.array([len(v) for v in named['inverse_transform']])
        if 'original_images' in named:
            out[key + "original_shapes"] = np.array([np.asarray(im).shape for im in named['original_images']])
        _state(out, key + "state")


SSD_RETURNS = {'processed_images', 'processed_labels', 'image_ids', 'filenames'}
EVAL_RETURNS = {'processed_images', 'image_ids', 'inverse_transform', 'original_labels', 'processed_labels'}
PLAIN_RETURNS = {'processed_images', 'processed_labels', 'filenames', 'image_ids', 'evaluation-neutral', 'inverse_transform',
                 'original_images', 'original_labels'}
PLAIN_LABELS = [[], [[1, 2, 3, 12, 14], [2, 5, 5, 5, 9]], [[3, 0, 0, 21, 17]], [[1, 4, 6, 10, 12], [2, 1, 1, 8, 3]]]


def run_ssd(ns, out, **generate_kw):
    np.random.seed(5)
    src = csv_generator(ns)
    g = ns.DataGenerator(load_images_into_memory=True, filenames=list(src.filenames), labels=list(src.labels), image_ids=list(src.image_ids),
                         verbose=False)
    gen = g.generate(batch_size=5, shuffle=True, transformations=[ns.SSDDataAugmentation(300, 300)], returns=SSD_RETURNS, **generate_kw)
    record_batches(out, "ssd", gen, SSD_RETURNS, 3)


def run_eval(ns, out, **generate_kw):
    np.random.seed(6)
    g = csv_generator(ns, load_images_into_memory=True, verbose=False)
    gen = g.generate(batch_size=4, shuffle=False, transformations=[ns.ConvertTo3Channels(), ns.Resize(300, 300)], returns=EVAL_RETURNS,
                     keep_images_without_gt=True, **generate_kw)
    record_batches(out, "eval", gen, EVAL_RETURNS, 3)


def run_plain(ns, out, **generate_kw):
    """transformations=[] on images of one size: an image without ground truth (removed; first in its batch -- the reference's removal
    bookkeeping pops its empty inverter list by index), a degenerate box (warned about), the epoch wrap."""
    np.random.seed(7)
    g = ns.DataGenerator(load_images_into_memory=True, filenames=[os.path.join(FIXTURES, n) for n, _ in EQUAL], labels=PLAIN_LABELS,
                         image_ids=['e%d' % i for i in range(4)], eval_neutral=[[False] * len(v) for v in PLAIN_LABELS], verbose=False)
    gen = g.generate(batch_size=3, shuffle=False, transformations=[], returns=PLAIN_RETURNS, degenerate_box_handling='warn', **generate_kw)
    record_batches(out, "plain", gen, PLAIN_RETURNS, 3)


def run_reference(ns):
    out = {}
    record_parsers(ns, out)
    run_plain(ns, out)
    run_ssd(ns, out)
    run_eval(ns, out)
    return out
