"""`ssdhip_eval_collect` / `ssdhip_eval_pack` (csrc/ssdhip_evalcollect.hip) against their NumPy statement tests/np_eval_collect.py, bit
for bit, at the smallest shapes that cross each boundary: a wave (64 rows), the collect workgroup (256 rows), the pack chunk (256
rows), the store's capacity.  Stores and outputs are sentinel-filled with a guard band behind them, and compared whole."""
import ctypes

import numpy as np
import pytest

from tests import np_eval_collect as ref

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = -777.0, 64
PROGRAMS = [[], [(0, 1.7, 0.61)], [(0, 0.37, 2.9), (1, -12.0, 5.0)], [(1, 3.0, -4.0), (0, 1.25, 0.8), (1, 0.0, 7.0), (0, 3.3, 1.1)]]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == 'f' else a


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def make_batch(rng, B, R, dtype, n_classes, counts, first_image, n_images):
    """rows (B, R, 6) with fractional coordinates and class-0 rows anywhere, count or None, desc with programs of 0, 1, 2 and 4 steps."""
    rows = np.zeros((B, R, 6))
    rows[:, :, 0] = rng.randint(0, n_classes + 1, size=(B, R))
    rows[:, :, 1] = rng.uniform(0, 1, size=(B, R))
    rows[:, :, 2:] = rng.uniform(-20, 320, size=(B, R, 4))
    if counts is not None:
        rows[:, :, 0] = np.where(rows[:, :, 0] == 0, 1, rows[:, :, 0])
    indices = [(first_image + b) % n_images for b in range(B)]
    desc = ref.make_desc(indices, [PROGRAMS[(first_image + b) % 4] for b in range(B)])
    return rows.astype(dtype), (None if counts is None else np.asarray(counts, dtype=np.int32)), desc


def run_collect(batches, capacity, dtype, n_images, n_classes, conf_decimals=0):
    """The batches appended one behind the other with no host read in between -> (rows, image, counters) downloaded, and the statement's store."""
    import torch
    from ssd_keras_amd import _native as nat
    want = ref.new_store(capacity, dtype, n_classes, fill=SENTINEL, guard=GUARD)
    rows_d = _dev(want["rows"].copy())
    image_d = _dev(want["image"].copy())
    counters = torch.full((nat.EVAL_COUNTERS,), 12345, dtype=torch.int32, device="cuda")
    nat.eval_store_reset(counters)
    for rows, count, desc in batches:
        nat.eval_collect(_dev(rows), None if count is None else _dev(count), _dev(desc), n_images, n_classes, 1, conf_decimals, rows_d,
                         image_d, counters, capacity=capacity)
        ref.collect(want, rows, count, desc, n_images, n_classes, 1, conf_decimals)
    return rows_d.cpu().numpy(), image_d.cpu().numpy(), counters.cpu().numpy(), want


def assert_store(got_rows, got_image, counters, want, n_classes):
    from ssd_keras_amd import _native as nat
    assert counters[nat.EVAL_N_ROWS] == want["n"] and counters[nat.EVAL_BAD_CLASS] == want["bad"] and counters[nat.EVAL_OVERFLOW] == want["overflow"]
    assert list(counters[nat.EVAL_CLASS_COUNT:nat.EVAL_CLASS_COUNT + n_classes]) == list(want["class_count"])
    assert not counters[nat.EVAL_CLASS_COUNT + n_classes:].any() and counters[3] == 0
    assert np.array_equal(_bits(got_rows), _bits(want["rows"]))
    assert np.array_equal(got_image, want["image"])
    assert (got_rows[want["capacity"]:] == SENTINEL).all() and (got_image[want["capacity"]:] == -7).all()


@pytest.mark.parametrize("n_appends", [2, 3])
@pytest.mark.parametrize("B,R", [(1, 1), (3, 64), (3, 65), (1, 200), (3, 257)])
@pytest.mark.parametrize("rule", ["count", "class"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_collect_equals_the_statement(dtype, rule, B, R, n_appends):
    rng = np.random.RandomState(R * 7 + B)
    n_images, n_classes = 11, 6
    batches = []
    for a in range(n_appends):
        counts = None if rule == "class" else [[0, 1, R][(a + b) % 3] for b in range(B)]
        batches.append(make_batch(rng, B, R, dtype, n_classes, counts, a * B, n_images))
    got = run_collect(batches, n_appends * B * R, dtype, n_images, n_classes, conf_decimals=4 if n_appends == 3 else 0)
    assert_store(*got, n_classes)
    assert got[3]["n"] > 0 or R == 1


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_capacity_reached_exactly_and_exceeded_by_one(dtype):
    rng = np.random.RandomState(5)
    n_images, n_classes, B, R = 4, 3, 2, 70
    batches = [make_batch(rng, B, R, dtype, n_classes, [R, 33], 0, n_images), make_batch(rng, B, R, dtype, n_classes, [1, R], 2, n_images)]
    total = R + 33 + 1 + R
    exact = run_collect(batches, total, dtype, n_images, n_classes)
    assert_store(*exact, n_classes)
    assert exact[3]["n"] == total and exact[3]["overflow"] == 0
    over = run_collect(batches, total - 1, dtype, n_images, n_classes)
    assert_store(*over, n_classes)
    assert over[3]["n"] == R + 33 and over[3]["overflow"] == 1
    assert (over[0][R + 33:] == SENTINEL).all()                  # the append that did not fit wrote nothing at all
    # the flag stays, and an append that fits again is taken
    again = run_collect(batches + [make_batch(rng, 1, R, dtype, n_classes, [1], 1, n_images)], total - 1, dtype, n_images, n_classes)
    assert_store(*again, n_classes)
    assert again[3]["n"] == R + 33 + 1 and again[3]["overflow"] == 1


@pytest.mark.parametrize("rule", ["count", "class"])
def test_out_of_range_classes_and_images_are_counted(rule):
    rng = np.random.RandomState(8)
    n_images, n_classes, B, R = 5, 4, 3, 20
    rows, count, desc = make_batch(rng, B, R, np.float64, n_classes, None if rule == "class" else [R, 7, R], 0, n_images)
    rows[0, 2, 0], rows[0, 5, 0], rows[1, 1, 0], rows[1, 3, 0], rows[2, 0, 0] = n_classes + 1, -3, 0.5, np.nan, 1e30
    desc[2, 0] = n_images                                        # an image index past the dataset: all its rows count as out of range
    got = run_collect([(rows, count, desc)], B * R, np.float64, n_images, n_classes)
    assert_store(*got, n_classes)
    assert got[3]["bad"] >= 5


def run_pack(store_rows, store_image, n, n_images, n_classes):
    import torch
    from ssd_keras_amd import _native as nat
    want = ref.pack(store_rows, store_image, n, n_images, n_classes)
    P = int(want[0].shape[0])
    outs = (torch.full((P + GUARD, 5), SENTINEL, dtype=torch.float32, device="cuda"), torch.full((P + GUARD,), -7, dtype=torch.int32, device="cuda"),
            torch.full((P + GUARD,), -7, dtype=torch.int32, device="cuda"), torch.full((n_classes + 1 + GUARD,), -7, dtype=torch.int32, device="cuda"))
    nat.eval_pack(_dev(store_rows), _dev(store_image), n, n_images, n_classes, out_rows=P, outputs=outs)
    got = [o.cpu().numpy() for o in outs]
    for g, size in zip(got, (P, P, P, n_classes + 1)):
        assert (g[size:] == (SENTINEL if g.dtype == np.float32 else -7)).all()
    return [g[:size] for g, size in zip(got, (P, P, P, n_classes + 1))], want


def make_store(rng, n, dtype, n_classes, n_images, classes=None, extra=3):
    rows = np.full((n + extra, 6), SENTINEL)
    rows[:n, 0] = rng.randint(1, n_classes + 1, size=n) if classes is None else classes
    rows[:n, 1] = rng.uniform(0, 1, size=n)
    rows[:n, 2:] = np.round(rng.uniform(-20, 520, size=(n, 4)), 1)
    image = np.full((n + extra,), -7, dtype=np.int32)
    image[:n] = np.sort(rng.randint(0, n_images, size=n))
    return rows.astype(dtype), image


@pytest.mark.parametrize("n_classes,one_class", [(1, False), (20, False), (80, False), (80, True)])
@pytest.mark.parametrize("n", [0, 1, ref.PACK_CHUNK - 1, ref.PACK_CHUNK, ref.PACK_CHUNK + 1, 2 * ref.PACK_CHUNK + 190])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_pack_equals_the_statement(dtype, n, n_classes, one_class):
    rng = np.random.RandomState(n + n_classes)
    n_images = 9
    rows, image = make_store(rng, n, dtype, n_classes, n_images, classes=min(37, n_classes) if one_class else None)
    got, want = run_pack(rows, image, n, n_images, n_classes)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(_bits(g), _bits(w))
    assert want[3][-1] == n
    again, _ = run_pack(rows, image, n, n_images, n_classes)      # the result does not depend on scheduling
    for g, a in zip(got, again):
        assert np.array_equal(_bits(g), _bits(a))


def test_pack_leaves_out_what_the_matcher_has_no_segment_for():
    rng = np.random.RandomState(12)
    n, n_classes, n_images = 600, 7, 5
    rows, image = make_store(rng, n, np.float64, n_classes, n_images)
    rows[[3, 255, 256, 511], 0] = [0, n_classes + 1, np.nan, -2]
    image[[17, 300]] = [n_images, -1]
    got, want = run_pack(rows, image, n, n_images, n_classes)
    assert want[0].shape[0] == n - 6
    for g, w in zip(got, want):
        assert np.array_equal(_bits(g), _bits(w))


def test_refusals_leave_every_output_untouched():
    import torch
    from ssd_keras_amd import _native as nat
    lib = nat.load()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    B, R, cap, C = 2, 5, 10, 3
    rows = torch.rand((B, R, 6), dtype=torch.float32, device="cuda")
    desc = torch.zeros((B, nat.EVAL_DESC), dtype=torch.float64, device="cuda")
    store = torch.full((cap, 6), SENTINEL, dtype=torch.float32, device="cuda")
    image = torch.full((cap,), -7, dtype=torch.int32, device="cuda")
    counters = torch.full((nat.EVAL_COUNTERS,), 12345, dtype=torch.int32, device="cuda")
    ws = torch.full((4096,), 9, dtype=torch.uint8, device="cuda")
    good = dict(rows=p(rows), dtype=nat.F32, B=B, R=R, count=None, desc=p(desc), n_images=4, n_classes=C, coord=1, conf=0, store=p(store),
                image=p(image), cap=cap, counters=p(counters), ws=p(ws), ws_bytes=4096)
    bad = [dict(dtype=2), dict(B=0), dict(B=1025), dict(R=0), dict(n_classes=0), dict(n_classes=nat.EVAL_MAX_CLASSES + 1), dict(n_images=0),
           dict(coord=10), dict(conf=-1), dict(cap=-1), dict(rows=None), dict(desc=None), dict(store=None), dict(image=None), dict(counters=None)]
    for change in bad:
        a = dict(good, **change)
        assert lib.ssdhip_eval_collect(*a.values(), None) == -1, change
    assert lib.ssdhip_eval_collect(*dict(good, ws_bytes=8).values(), None) == -2
    assert lib.ssdhip_eval_store_reset(None, None) == -1
    pred = torch.full((cap, 5), SENTINEL, dtype=torch.float32, device="cuda")
    seg, slot, starts = (torch.full((cap,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    need = lib.ssdhip_eval_pack_workspace_bytes(cap, C)
    assert need > 0 and lib.ssdhip_eval_pack_workspace_bytes(-1, C) == 0 and lib.ssdhip_eval_pack_workspace_bytes(cap, 129) == 0
    wsp = torch.full((need,), 9, dtype=torch.uint8, device="cuda")
    goodp = dict(store=p(store), dtype=nat.F32, image=p(image), n=cap, n_images=4, n_classes=C, pred=p(pred), seg=p(seg), slot=p(slot),
                 starts=p(starts), out_rows=cap, ws=p(wsp), ws_bytes=need)
    badp = [dict(dtype=-1), dict(n=-1), dict(n_images=0), dict(n_classes=0), dict(n_classes=129), dict(out_rows=-1), dict(store=None),
            dict(image=None), dict(pred=None), dict(seg=None), dict(slot=None), dict(starts=None), dict(n_images=1 << 30, n_classes=4)]
    for change in badp:
        assert lib.ssdhip_eval_pack(*dict(goodp, **change).values(), None) == -1, change
    assert lib.ssdhip_eval_pack(*dict(goodp, ws_bytes=need - 1).values(), None) == -2
    torch.cuda.synchronize()
    assert (store == SENTINEL).all() and (pred == SENTINEL).all() and (counters == 12345).all() and (ws == 9).all() and (wsp == 9).all()
    for t in (image, seg, slot, starts):
        assert (t == -7).all()
