"""What the augmentation chains share on the host (ssd_keras_amd/data_generator/_chain_batch.py) and the one decision wrapper behind
`_native`'s five public ones, without a GPU: label buffers, the batch argument parser, np.random's state in the kernels' layout, and the
packed upload / download of every decision export with `nat.launch` replaced by a recorder."""
import ctypes

import numpy as np
import pytest

from ssd_keras_amd import _native as nat
from ssd_keras_amd.data_generator import _chain_batch as cb


# ---- labels ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int64, np.float64])
def test_labels_round_trip_through_the_kernels_buffer(dtype):
    labels_format = {'xmin': 0, 'ymin': 1, 'xmax': 2, 'ymax': 3, 'class_id': 4}            # the class behind the corners
    cols = cb.label_cols(labels_format)
    assert cols == [4, 0, 1, 2, 3]
    rng = np.random.RandomState(3)
    labels = [rng.randint(0, 500, size=(n, 5)).astype(dtype) for n in (0, 1, nat.AUG_MAX_BOXES)]
    assert cb.labels_fit(labels)
    arrs, lab_in, n_in = cb.pack_labels(labels, cols)
    assert lab_in.shape == (3, nat.AUG_MAX_BOXES, 5) and lab_in.dtype == np.float64
    assert n_in.dtype == np.int32 and n_in.tolist() == [0, 1, nat.AUG_MAX_BOXES]
    assert all(a.dtype == dtype for a in arrs)
    for a, rows, n in zip(labels, lab_in, n_in):
        assert np.array_equal(rows[:n, 0], a[:, 4]) and np.array_equal(rows[:n, 1:], a[:, :4])        # class, xmin, ymin, xmax, ymax
        assert not rows[n:].any()
    back = cb.unpack_labels(lab_in, n_in, cols, arrs[0].dtype)
    assert len(back) == 3
    for a, b in zip(labels, back):
        assert b.dtype == a.dtype and b.shape == a.shape and np.array_equal(a, b) and b.flags.c_contiguous


def test_the_label_layout_predicate():
    ok = np.array([[1, 2, 3, 40, 50]], dtype=np.int64)
    assert cb.labels_fit([ok, np.zeros((0, 5), dtype=np.int64)])
    assert cb.labels_fit([np.tile(ok, (nat.AUG_MAX_BOXES, 1))])
    assert not cb.labels_fit([np.tile(ok, (nat.AUG_MAX_BOXES + 1, 1))])                     # 65 rows
    assert not cb.labels_fit([ok, ok.astype(np.float64)])                                   # mixed dtypes
    assert not cb.labels_fit([ok.astype(np.float32)])
    assert not cb.labels_fit([ok[:, :4]])                                                   # (n, 4)


# ---- augment_batch's arguments ------------------------------------------------------------------------------------------------------
def test_the_batch_parser_raises_what_the_chains_raised():
    import torch
    img = np.zeros((8, 9, 3), dtype=np.uint8)
    lab = np.zeros((0, 5), dtype=np.int64)
    with pytest.raises(TypeError) as e:
        cb.parse_batch([img, np.zeros((8, 9, 1), dtype=np.uint8)], [lab, lab])
    assert str(e.value) == "augment_batch takes a list of (H, W, 3) uint8 images"
    with pytest.raises(TypeError) as e:
        cb.parse_batch(torch.zeros((2, 8, 9, 3), dtype=torch.uint8), [lab, lab])            # a CPU tensor
    assert str(e.value) == "augment_batch takes a list of (H, W, 3) uint8 images or a (B, H, W, 3) CUDA uint8 batch"
    with pytest.raises(TypeError) as e:
        cb.parse_batch(torch.zeros((2, 8, 9, 3), dtype=torch.uint8), [lab, lab], lists=False)
    assert str(e.value) == "augment_batch takes a (B, H, W, 3) CUDA uint8 batch"
    with pytest.raises(TypeError) as e:
        cb.parse_batch([img, img], [lab, lab], lists=False)                                 # a list, to a chain that takes none
    assert str(e.value) == "augment_batch takes a (B, H, W, 3) CUDA uint8 batch"
    with pytest.raises(ValueError) as e:
        cb.parse_batch([img, img], [lab])
    assert str(e.value) == "one label array per image"


def test_the_batch_parser_counts_seeds_and_returns_the_shapes(monkeypatch):
    from ssd_keras_amd.data_generator import _image_ops as iop

    class Packed:
        shapes = [(8, 9, 3), (5, 7, 3)]
    monkeypatch.setattr(iop, "pack_ragged", lambda images: Packed)                          # looked up at call time, as the CPU suites need
    images = [np.zeros(s, dtype=np.uint8) for s in Packed.shapes]
    lab = np.zeros((0, 5), dtype=np.int64)
    with pytest.raises(ValueError) as e:
        cb.parse_batch(images, [lab, lab], seeds=[1, 2, 3])
    assert str(e.value) == "one seed per image"
    assert cb.parse_batch(images, [lab, lab], seeds=[1, 2]) == (None, Packed, [(8, 9), (5, 7)])


# ---- np.random's state --------------------------------------------------------------------------------------------------------------
def test_the_state_helpers_round_trip_np_random():
    np.random.seed(11)
    np.random.uniform(size=7)
    np.random.normal()                                                                      # leaves a cached gauss in the state's tail
    before = np.random.get_state()
    name, mt, rest = cb.read_np_state()
    assert name == 'MT19937' and mt.shape == (625,) and mt.dtype == np.uint32
    assert np.array_equal(mt[:624], before[1]) and int(mt[624]) == before[2] and tuple(rest) == tuple(before[3:])
    np.random.seed(99)
    cb.put_np_state(name, mt, rest)
    after = np.random.get_state()
    assert after[0] == before[0] and np.array_equal(after[1], before[1]) and after[2:] == before[2:]
    # a state that has moved on (what a decision kernel hands back): the stream continues where an untouched generator would be
    rs = np.random.RandomState()
    rs.set_state(before)
    rs.uniform(size=1000)                                                                   # across a twist of the key
    st = rs.get_state()
    moved = np.empty((625,), dtype=np.uint32)
    moved[:624], moved[624] = st[1], st[2]
    cb.put_np_state(name, moved, st[3:])
    assert [np.random.uniform() for _ in range(10)] == [rs.uniform() for _ in range(10)]
    states = np.zeros((2, 625), dtype=np.uint32)
    cb.record_np_state(states, 1)
    now = np.random.get_state()
    assert not states[0].any() and np.array_equal(states[1, :624], now[1]) and int(states[1, 624]) == now[2]


# ---- the decision wrapper's packed buffers ------------------------------------------------------------------------------------------
B = 2
_I32, _F64, _U32 = np.dtype(np.int32), np.dtype(np.float64), np.dtype(np.uint32)
# export, the structs in front, scalars behind B, ragged table?, turns?, mt_states' shape, geometry (dtype, columns), programs?
FAMILIES = [
    ("ssdhip_ssd_augment_decide", [nat._AugParams], 0, False, False, (B, 625), (_I32, 12), False),
    ("ssdhip_ssd_augment_decide_stream", [nat._AugParams, nat._AugPhoto], 0, False, False, (625,), (_I32, 12), True),
    ("ssdhip_ssd_augment_decide_stream_ragged", [nat._AugParams, nat._AugPhoto], 0, True, False, (625,), (_I32, 12), True),
    ("ssdhip_const_augment_decide", [nat._ConstAugParams], 0, False, False, (B, 625), (_F64, nat.CONST_AUG_GEO), True),
    ("ssdhip_const_augment_decide_stream", [nat._ConstAugParams], 0, False, False, (625,), (_F64, nat.CONST_AUG_GEO), True),
    ("ssdhip_var_augment_decide", [nat._VarAugParams], 1, True, False, (B, 625), (_I32, 12), True),
    ("ssdhip_var_augment_decide_stream", [nat._VarAugParams], 1, False, False, (625,), (_I32, 12), True),
    ("ssdhip_var_augment_decide_stream_ragged", [nat._VarAugParams], 1, True, False, (625,), (_I32, 12), True),
    ("ssdhip_sat_augment_decide", [nat._SatAugParams], 1, True, True, (B, 625), (_I32, 12), True),
    ("ssdhip_sat_augment_decide_stream", [nat._SatAugParams], 1, False, True, (625,), (_I32, 12), True),
    ("ssdhip_sat_augment_decide_stream_ragged", [nat._SatAugParams], 1, True, True, (625,), (_I32, 12), True),
]


class _Recorder:
    """`nat.launch` and the two allocations of `nat._decide` (torch.from_numpy: the upload, torch.empty: the download), recorded."""

    def __init__(self, monkeypatch):
        import torch
        self.launches, self.uploads, self.downloads = [], [], []
        rec = self

        class Torch:
            def __getattr__(self, name):
                return getattr(torch, name)

            def from_numpy(self, a):
                rec.uploads.append(torch.from_numpy(a))
                return rec.uploads[-1]

            def empty(self, *args, **kwargs):
                rec.downloads.append(torch.empty(*args, **kwargs))
                return rec.downloads[-1]
        proxy = Torch()
        monkeypatch.setattr(nat, "_torch", lambda: proxy)
        monkeypatch.setattr(nat, "launch", lambda name, device, *args: self.launches.append((name, device, args)))


def _inside(ptr, nbytes, buf):
    return buf.data_ptr() <= ptr and ptr + nbytes <= buf.data_ptr() + buf.numel()


@pytest.mark.parametrize("family", FAMILIES, ids=[f[0][len("ssdhip_"):] for f in FAMILIES])
def test_decision_wrapper_layout(monkeypatch, family):
    """`nat._decide`, driven once per export on CPU tensors (it makes no CUDA check of its own; the public wrappers validate the ragged
    table before they reach it): the export and its argument list, every pointer inside the one upload or the one download and aligned
    to its element, the input sections holding what went in, and each output section coming back from fetch() and the device views
    under its own name, shape and dtype."""
    import torch
    export, structs, n_scalars, ragged, turned, mt_shape, (geo_dt, geo_cols), programs = family
    rec = _Recorder(monkeypatch)
    rng = np.random.RandomState(len(export))
    mt = rng.randint(0, 2 ** 32, size=mt_shape, dtype=np.uint64).astype(np.uint32)
    labels = rng.uniform(0, 300, size=(B, nat.AUG_MAX_BOXES, 5))
    n_labels = np.array([3, 64], dtype=np.int32)
    turns = np.array([3, 1], dtype=np.int32) if turned else None
    table = torch.from_numpy(np.array([[0, 8, 9, 3], [256, 5, 7, 3]], dtype=np.int64))
    qs = [s() for s in structs]
    lead = [ctypes.byref(q) for q in qs] + [B] + [64] * n_scalars + ([nat._ptr(table)] if ragged else [])
    ops_dev, args_dev, geo_dev, fetch = nat._decide(export, lead, mt, labels, n_labels, "cpu", geo_dt, geo_cols, "bad shapes",
                                                    programs=programs, turns=turns)
    assert len(rec.launches) == 1 and len(rec.uploads) == 1 and len(rec.downloads) == 1
    name, device, args = rec.launches[0]
    up, down = rec.uploads[0], rec.downloads[0]
    assert name == export and device == "cpu"

    # ---- the argument list: structs, B, scalars, then nothing but pointers; as many as the C prototype has in front of the stream
    assert list(args[:len(lead)]) == lead
    ptrs = args[len(lead):]
    assert all(isinstance(p, ctypes.c_void_p) and p.value for p in ptrs)
    _, argtypes = nat.SIGNATURES[export]
    assert len(args) == len(argtypes) - 1                                                   # the stream is `launch`'s to add
    assert all(t is ctypes.c_void_p for t in argtypes[len(structs) + 1 + n_scalars:])
    assert all(t is ctypes.c_int for t in argtypes[len(structs):len(structs) + 1 + n_scalars])

    # ---- their order is the export's: [turns,] mt, labels, n, [ops, args,] geometry, labels_out, n_out, mt_out
    inputs = ([("turns", _I32, (B,), turns)] if turned else []) + [("mt", _U32, mt_shape, mt), ("labels", _F64, labels.shape, labels),
                                                                    ("n", _I32, (B,), n_labels)]
    outputs = ([("ops", _I32, (B, nat.IMG_PROG)), ("args", _F64, (B, nat.IMG_PROG))] if programs else []) + [
        ("geometry", geo_dt, (B, geo_cols)), ("labels_out", _F64, (B, nat.AUG_MAX_BOXES, 5)), ("n_out", _I32, (B,)), ("mt_out", _U32, mt_shape)]
    assert len(ptrs) == len(inputs) + len(outputs)
    spans = []
    for p, (what, dt, shape, value) in zip(ptrs, inputs):
        nbytes = int(np.prod(shape)) * dt.itemsize
        assert _inside(p.value, nbytes, up), what
        assert (p.value - up.data_ptr()) % dt.itemsize == 0 and p.value % dt.itemsize == 0, what
        assert np.array_equal(np.frombuffer(ctypes.string_at(p.value, nbytes), dtype=dt).reshape(shape), value), what
        spans.append((p.value, p.value + nbytes))
    want = {}
    for k, (p, (what, dt, shape)) in enumerate(zip(ptrs[len(inputs):], outputs)):
        nbytes = int(np.prod(shape)) * dt.itemsize
        assert _inside(p.value, nbytes, down), what
        assert (p.value - down.data_ptr()) % dt.itemsize == 0 and p.value % dt.itemsize == 0, what
        want[what] = (np.arange(int(np.prod(shape))) * (k + 2) + 1000 * (k + 1)).astype(dt).reshape(shape)       # one pattern per section
        ctypes.memmove(p.value, want[what].tobytes(), nbytes)
        spans.append((p.value, p.value + nbytes))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), "sections overlap"

    # ---- fetch(): (geometry, labels_out, n_out, mt_out); the device views: ops, args, geometry
    got = dict(zip(("geometry", "labels_out", "n_out", "mt_out"), fetch()))
    for what, dt, shape in outputs[-4:]:
        assert got[what].dtype == dt and got[what].shape == tuple(shape) and np.array_equal(got[what], want[what]), what
    views = {"geometry": geo_dev}
    if programs:
        views.update(ops=ops_dev, args=args_dev)
    else:
        assert ops_dev is None and args_dev is None
    for what, view in views.items():
        assert _inside(view.data_ptr(), view.numel() * view.element_size(), down), what
        assert view.numpy().dtype == want[what].dtype and np.array_equal(view.numpy(), want[what]), what


def test_decision_wrappers_keep_their_messages(monkeypatch):
    """The public wrappers in front of `_decide`: each refuses arrays of the wrong shape with its own text, ahead of any launch."""
    rec = _Recorder(monkeypatch)
    labels = np.zeros((B, nat.AUG_MAX_BOXES, 5))
    n = np.zeros((B,), dtype=np.int32)
    seeded, stream, bad = np.zeros((B, 625), dtype=np.uint32), np.zeros((625,), dtype=np.uint32), np.zeros((B, 624), dtype=np.uint32)
    photo = dict(prob=[0.5] * 4, lower=[0.0] * 4, upper=[1.0] * 4, swap_prob=0.0)
    for call, text in (
            (lambda: nat.ssd_augment_decide({}, stream, labels, n, "cpu"), "ssd_augment_decide: mt_states (B, 625), labels (B, 64, 5), n_labels (B,)"),
            (lambda: nat.ssd_augment_decide_stream({}, photo, seeded, labels, n, "cpu"),
             "ssd_augment_decide_stream: mt_state (625,), labels (B, 64, 5), n_labels (B,)"),
            (lambda: nat.const_augment_decide({}, bad, labels, n, "cpu"),
             "const_augment_decide: mt_states (B, 625) or (625,), labels (B, 64, 5), n_labels (B,)"),
            (lambda: nat.var_augment_decide({}, seeded, labels[:, :10], n, "cpu"),
             "var_augment_decide: mt_states (B, 625) or (625,), labels (B, 64, 5), n_labels (B,)"),
            (lambda: nat.sat_augment_decide({}, [1, 2], stream, labels, n[:1], "cpu"),
             "sat_augment_decide: mt_states (B, 625) or (625,), labels (B, 64, 5), n_labels (B,)"),
            (lambda: nat.sat_augment_decide({}, [1, 4], stream, labels, n, "cpu"), "sat_augment_decide: turns (B,) with values 1 .. 3")):
        with pytest.raises(nat.SsdHipError) as e:
            call()
        assert str(e.value) == text
    assert not rec.launches and not rec.uploads
    # ... and fills the satellite's nested struct through the one filler: the two outer fields outside, the rest in `.var`
    q = nat._fill_struct(nat._SatAugParams(), dict(vflip_prob=0.25, rotate_prob=0.75, flip_prob=0.5, photo_prob=[0.1, 0.2, 0.3, 0.4], n_trials=3),
                         inner="var")
    assert (q.vflip_prob, q.rotate_prob, q.var.flip_prob, list(q.var.photo_prob), q.var.n_trials) == (0.25, 0.75, 0.5, [0.1, 0.2, 0.3, 0.4], 3)
    assert nat.ssd_augment_decide_stream({}, photo, stream, labels, n, "cpu")[3] is not None and rec.launches[0][0] == "ssdhip_ssd_augment_decide_stream"
    assert list(rec.launches[0][2][1]._obj.prob) == [0.5] * 4
