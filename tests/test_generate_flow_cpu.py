"""The control flow of DataGenerator.generate() with a non-empty transformation list, without a GPU: five in-memory 4 x 5 x 3 images and
stub transforms that are plain callables (no batch path takes them, so everything is the per-image loop unless a test patches the path).
What is pinned: the removal of items without ground truth from every return, the inverters' order, the order of the yielded list, the
returns without labels, the degenerate-box warning, the reference's None-image quirk, the epoch wrap, the row bookkeeping of a batch path
(`_batch_path` and `_transform_batch` patched to CPU stand-ins), the fallback of 'program' to the loop, and how often a batch's path is
decided."""
import warnings
from copy import deepcopy

import numpy as np
import pytest

from ssd_keras_amd.data_generator import object_detection_2d_data_generator as odg

ALL_RETURNS = {'processed_images', 'encoded_labels', 'matched_anchors', 'processed_labels', 'filenames', 'image_ids', 'evaluation-neutral',
               'inverse_transform', 'original_images', 'original_labels'}
# item 1 has an empty label array: no ground truth; item k's image is filled with VALUES[k]
LABELS = [[[1, 0, 0, 3, 2]], np.zeros((0, 5), dtype=np.int64), [[2, 1, 1, 4, 3], [3, 0, 1, 2, 2]], [[1, 2, 0, 5, 4]], [[3, 1, 2, 3, 4]]]
VALUES = [10, 20, 30, 40, 50]


def _generator(labels=LABELS):
    g = odg.DataGenerator(labels=deepcopy(labels) if labels is not None else None, image_ids=['id%d' % k for k in range(5)],
                          eval_neutral=[[False] * len(l) for l in labels] if labels is not None else None, verbose=False)
    g.images = [np.full((4, 5, 3), v, dtype=np.uint8) for v in VALUES]
    g.filenames = ['file%d' % k for k in range(5)]
    g.dataset_size, g.dataset_indices = 5, np.arange(5, dtype=np.int32)
    return g


class AddOne:
    """Adds 1 to the image; accepts `return_inverter` (its inverter names the stub and the value it produced)."""

    def __init__(self, tag):
        self.tag, self.calls = tag, []

    def __call__(self, image, labels=None, return_inverter=False):
        self.calls.append((labels is not None, return_inverter))
        image = image + np.uint8(1)
        out = (image,) + ((labels,) if labels is not None else ()) + (((self.tag, int(image[0, 0, 0])),) if return_inverter else ())
        return out if len(out) > 1 else image


class Double:
    """Doubles the image; does not accept `return_inverter`."""

    def __init__(self):
        self.calls = []

    def __call__(self, image, labels=None):
        self.calls.append(labels is not None)
        image = image * np.uint8(2)
        return image if labels is None else (image, labels)


def _stubs():
    return [AddOne('a'), Double(), AddOne('b')]                      # value v -> 2 (v + 1) + 1


def _after(v):
    return 2 * (v + 1) + 1


def _encoder(batch_y, diagnostics=False):
    return ('encoded', len(batch_y), diagnostics)


def _all_returns(g, **kw):
    """One batch of five with every return -> (the yielded list, the warnings' texts)."""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        got = next(g.generate(batch_size=5, shuffle=False, returns=ALL_RETURNS, **kw))
    return got, [str(w.message) for w in caught]


def _rows(images, values):
    assert isinstance(images, np.ndarray) and images.dtype == np.uint8 and images.shape == (len(values), 4, 5, 3)
    assert [int(v) for v in images[:, 0, 0, 0]] == list(values) and all((im == im[0, 0, 0]).all() for im in images)


def test_loop_removes_items_without_ground_truth_and_orders_inverters_and_returns():
    stubs = _stubs()
    got, texts = _all_returns(_generator(), transformations=stubs, label_encoder=_encoder)
    assert len(got) == 10
    images, encoded, anchors, labels, filenames, ids, neutral, inverters, original_images, original_labels = got
    keep = [0, 2, 3, 4]
    _rows(images, [_after(VALUES[k]) for k in keep])
    assert encoded == ('encoded', 4, False) and anchors is None
    assert any("not an `SSDInputEncoder`" in t for t in texts)
    assert len(labels) == 4 and all(isinstance(l, np.ndarray) for l in labels)
    for l, k in zip(labels, keep):
        np.testing.assert_array_equal(l, np.array(LABELS[k]))
    assert filenames == ['file%d' % k for k in keep] and ids == ['id%d' % k for k in keep]
    assert neutral == [[False] * len(LABELS[k]) for k in keep]
    # per item, the last transform's inverter first; the stub without `return_inverter` contributes none
    assert inverters == [[('b', _after(VALUES[k])), ('a', VALUES[k] + 1)] for k in keep]
    assert len(original_images) == 4
    for im, k in zip(original_images, keep):
        np.testing.assert_array_equal(im, np.full((4, 5, 3), VALUES[k], dtype=np.uint8))
    assert original_labels == [LABELS[k] for k in keep]               # lists, as the dataset holds them
    # the item without ground truth never reached a transform; every call had labels, the inverter was asked of those that take it
    assert stubs[0].calls == [(True, True)] * 4 and stubs[1].calls == [True] * 4 and stubs[2].calls == [(True, True)] * 4


def test_loop_asks_for_no_inverter_unless_it_is_returned():
    stubs = _stubs()
    g = _generator()
    images, labels = next(g.generate(batch_size=5, shuffle=False, transformations=stubs, returns={'processed_images', 'processed_labels'}))
    _rows(images, [_after(VALUES[k]) for k in (0, 2, 3, 4)])
    assert len(labels) == 4 and stubs[0].calls == [(True, False)] * 4


def test_keep_images_without_gt_keeps_the_item():
    stubs = _stubs()
    got, _ = _all_returns(_generator(), transformations=stubs, label_encoder=_encoder, keep_images_without_gt=True)
    images, encoded, anchors, labels, filenames, ids, neutral, inverters, original_images, original_labels = got
    _rows(images, [_after(v) for v in VALUES])
    assert encoded == ('encoded', 5, False)
    assert labels[1].size == 0 and filenames == ['file%d' % k for k in range(5)] and ids == ['id%d' % k for k in range(5)]
    assert neutral[1] == [] and len(neutral) == 5 and len(original_images) == 5
    assert len(original_labels) == 5 and original_labels[1].shape == (0, 5) and original_labels[2] == LABELS[2]
    assert inverters == [[('b', _after(v)), ('a', v + 1)] for v in VALUES]
    assert stubs[0].calls == [(True, True)] * 5


def test_without_labels_transforms_get_the_image_only_and_label_returns_are_none():
    stubs = _stubs()
    got, texts = _all_returns(_generator(labels=None), transformations=stubs, label_encoder=_encoder)
    images, encoded, anchors, labels, filenames, ids, neutral, inverters, original_images, original_labels = got
    _rows(images, [_after(v) for v in VALUES])
    assert encoded is None and anchors is None and labels is None and neutral is None and original_labels is None
    assert any("Since no labels were given" in t for t in texts)
    assert filenames == ['file%d' % k for k in range(5)] and ids == ['id%d' % k for k in range(5)] and len(original_images) == 5
    assert inverters == [[('b', _after(v)), ('a', v + 1)] for v in VALUES]
    assert stubs[0].calls == [(False, True)] * 5 and stubs[1].calls == [False] * 5
    assert not any(hasattr(s, 'labels_format') for s in stubs)          # set only when there are labels


def test_degenerate_box_warns_and_stays():
    labels = deepcopy(LABELS)
    labels[3] = [[1, 2, 0, 2, 4], [2, 0, 0, 3, 3]]                     # xmax == xmin
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        images, got = next(_generator(labels).generate(batch_size=5, shuffle=False, transformations=_stubs(),
                                                       returns={'processed_images', 'processed_labels'}, degenerate_box_handling='warn'))
    texts = [str(w.message) for w in caught if "degenerate" in str(w.message)]
    assert len(texts) == 1 and "batch item 3" in texts[0]
    assert len(images) == 4
    np.testing.assert_array_equal(got[2], np.array(labels[3]))


class DropImage:
    def __call__(self, image, labels=None):
        return None if labels is None else (None, labels)


def test_a_none_image_with_labels_ends_in_type_error():
    """The reference's quirk (its `continue` at :1076-1079 only continues the loop over the transforms): pinned, not fixed."""
    gen = _generator().generate(batch_size=5, shuffle=False, transformations=[AddOne('a'), DropImage(), AddOne('b')],
                                returns={'processed_images', 'processed_labels'})
    with pytest.raises(TypeError):
        next(gen)
    with pytest.raises(StopIteration):                                  # nothing was, nothing will be yielded
        next(gen)


class DropValue:
    """Drops the image whose pixels have this value, keeps its labels."""

    def __init__(self, value):
        self.value = value

    def __call__(self, image, labels=None):
        return (None if int(image[0, 0, 0]) == self.value else image), labels


def test_a_none_image_from_the_last_transform_removes_the_item_and_leaves_its_inverters():
    """The other half of that quirk (:1076-1078, :1089): the item leaves the batch, but the reference has appended both a [] and the
    item's own inverters to its one list, and the removal pops one entry per item -- so the list keeps one entry too many and is
    misaligned behind the dropped item.  Pinned, not fixed."""
    images, labels, filenames, inverters = next(_generator().generate(
        batch_size=5, shuffle=False, transformations=[AddOne('a'), DropValue(41)],
        returns={'processed_images', 'processed_labels', 'filenames', 'inverse_transform'}))
    _rows(images, [11, 31, 51])
    assert filenames == ['file0', 'file2', 'file4'] and len(labels) == 3
    assert inverters == [[('a', 11)], [('a', 31)], [('a', 41)], [('a', 51)]]


def test_without_transformations_the_inverter_list_holds_the_items_without_ground_truth_only():
    """The reference appends to its list of inverters per item only when there are transformations, but a [] for every item without
    ground truth either way (:1058), and pops that list at the removed items' batch indices (:1123): fine when the item is the first of
    its batch (tests/test_data_generator_cpu.py), IndexError when it is not.  Pinned, not fixed."""
    gen = _generator().generate(batch_size=5, shuffle=False, transformations=[], returns={'processed_images', 'inverse_transform'})
    with pytest.raises(IndexError, match="pop index out of range"):
        next(gen)
    first = deepcopy(LABELS)
    first[0], first[1] = first[1], first[0]
    images, inverters = next(_generator(first).generate(batch_size=5, shuffle=False, transformations=[],
                                                        returns={'processed_images', 'inverse_transform'}))
    _rows(images, VALUES[1:])
    assert inverters == []


def test_removal_needs_file_names():
    """The reference pops the batch's file names unconditionally (:1122): images in memory without file names cannot lose an item."""
    g = _generator()
    g.filenames = None
    with pytest.raises(AttributeError):
        next(g.generate(batch_size=5, shuffle=False, transformations=_stubs(), returns={'processed_images'}))


def test_epoch_wrap():
    labels = deepcopy(LABELS)
    labels[1] = [[1, 0, 0, 2, 2]]
    gen = _generator(labels).generate(batch_size=2, shuffle=False, transformations=[AddOne('a')], returns={'processed_images', 'filenames'})
    batches = [next(gen) for _ in range(4)]
    assert [b[1] for b in batches] == [['file0', 'file1'], ['file2', 'file3'], ['file4'], ['file0', 'file1']]
    for (images, _), values in zip(batches, ([10, 20], [30, 40], [50], [10, 20])):
        _rows(images, [v + 1 for v in values])


class _BatchStub:
    """Stands in for `_transform_batch`: a CPU tensor whose row k is the k-th image it was given + 100, the labels it was given (the
    item of value `degenerate` gets a degenerate first box), one inverter per item."""

    def __init__(self, degenerate=None, error=None):
        self.calls, self.degenerate, self.error = [], degenerate, error

    def __call__(self, generator, path, transformations, images, labels, want_inverters, warps=False):
        import torch
        values = [int(im[0, 0, 0]) for im in images]
        self.calls.append((path, values, None if labels is None else [np.array(l) for l in labels], want_inverters, warps))
        if self.error is not None:
            raise self.error
        out_labels = None
        if labels is not None:
            out_labels = [np.array(l) for l in labels]
            for l, v in zip(out_labels, values):
                if v == self.degenerate:
                    l[0, 3] = l[0, 1]
        batch = torch.from_numpy(np.stack([np.full((2, 2, 3), v + 100, dtype=np.uint8) for v in values]))
        return batch, out_labels, [[('batch', v)] for v in values]


class _CpuBoxFilter:
    """BoxFilter(check_degenerate=True) in NumPy (the package's runs on the device)."""

    def __init__(self, labels_format, **kw):
        self.f = labels_format

    def __call__(self, labels):
        f = self.f
        return labels[(labels[:, f['xmax']] > labels[:, f['xmin']]) & (labels[:, f['ymax']] > labels[:, f['ymin']])]


def _patch_path(monkeypatch, path, stub):
    monkeypatch.setattr(odg.DataGenerator, "_batch_path", staticmethod(lambda transformations, images, have_labels: path))
    monkeypatch.setattr(odg.DataGenerator, "_transform_batch", lambda self, *a, **kw: stub(self, *a, **kw))


RETURNS = {'processed_images', 'processed_labels', 'filenames', 'inverse_transform'}


def test_batch_path_rows_follow_the_survivors(monkeypatch):
    stub = _BatchStub(degenerate=40)
    _patch_path(monkeypatch, 'gather', stub)
    monkeypatch.setattr(odg, "BoxFilter", _CpuBoxFilter)
    stubs = _stubs()
    images, labels, filenames, inverters = next(_generator().generate(batch_size=5, shuffle=False, transformations=stubs, returns=RETURNS))
    # the item without ground truth never reaches the batch path; no transform is called outside it
    assert len(stub.calls) == 1
    path, values, given, want_inverters, warps = stub.calls[0]
    assert (path, values, want_inverters, warps) == ('gather', [10, 30, 40, 50], True, False)
    for l, k in zip(given, (0, 2, 3, 4)):
        np.testing.assert_array_equal(l, np.array(LABELS[k]))
    assert not any(s.calls for s in stubs)
    # item 3's only box became degenerate and was removed, so its row is dropped too: rows 0, 1, 3 of the stub's batch
    assert isinstance(images, np.ndarray) and images.shape == (3, 2, 2, 3) and images.dtype == np.uint8
    assert [int(v) for v in images[:, 0, 0, 0]] == [110, 130, 150]
    assert filenames == ['file0', 'file2', 'file4'] and inverters == [[('batch', 10)], [('batch', 30)], [('batch', 50)]]
    for l, k in zip(labels, (0, 2, 4)):
        np.testing.assert_array_equal(l, np.array(LABELS[k]))


def test_batch_path_keeps_every_row_when_nothing_is_removed(monkeypatch):
    stub = _BatchStub(degenerate=30)                                    # item 2 keeps its second box
    _patch_path(monkeypatch, 'gather', stub)
    monkeypatch.setattr(odg, "BoxFilter", _CpuBoxFilter)
    images, labels, filenames, inverters = next(_generator().generate(batch_size=5, shuffle=False, transformations=_stubs(), returns=RETURNS,
                                                                      keep_images_without_gt=True))
    assert stub.calls[0][1] == VALUES
    assert [int(v) for v in images[:, 0, 0, 0]] == [v + 100 for v in VALUES] and filenames == ['file%d' % k for k in range(5)]
    assert inverters == [[('batch', v)] for v in VALUES]
    assert labels[1].size == 0
    np.testing.assert_array_equal(labels[2], np.array(LABELS[2][1:]))


def test_program_falls_back_to_the_loop_and_gather_does_not(monkeypatch):
    stub = _BatchStub(error=NotImplementedError("cannot compose"))
    _patch_path(monkeypatch, 'program', stub)
    stubs = _stubs()
    images, labels, filenames, inverters = next(_generator().generate(batch_size=5, shuffle=False, transformations=stubs, returns=RETURNS))
    assert len(stub.calls) == 1 and stub.calls[0][0] == 'program'
    # the loop's batch: the item without ground truth removed once (a doubled removal would drop file4 too, or fail)
    keep = [0, 2, 3, 4]
    _rows(images, [_after(VALUES[k]) for k in keep])
    assert filenames == ['file%d' % k for k in keep] and len(labels) == 4
    assert inverters == [[('b', _after(VALUES[k])), ('a', VALUES[k] + 1)] for k in keep]
    assert stubs[0].calls == [(True, True)] * 4

    _patch_path(monkeypatch, 'gather', stub)
    with pytest.raises(NotImplementedError, match="cannot compose"):
        next(_generator().generate(batch_size=5, shuffle=False, transformations=_stubs(), returns=RETURNS))


def _spy(monkeypatch):
    """`_batch_path` counted per call, answering as before."""
    calls, real = [], odg.DataGenerator.__dict__['_batch_path'].__func__

    def spy(transformations, images, have_labels):
        calls.append(len(images))
        return real(transformations, images, have_labels)
    monkeypatch.setattr(odg.DataGenerator, "_batch_path", staticmethod(spy))
    return calls


def test_path_is_decided_once_per_batch_in_memory(monkeypatch):
    calls = _spy(monkeypatch)
    gen = _generator().generate(batch_size=2, shuffle=False, transformations=_stubs(), returns={'processed_images'})
    for n in range(1, 4):
        next(gen)
        assert len(calls) == n
    gen = _generator().generate(batch_size=2, shuffle=False, transformations=[], returns={'processed_images'}, keep_images_without_gt=True)
    next(gen)
    assert len(calls) == 3                                              # an empty list has no path to decide


def test_path_is_decided_once_per_batch_with_device_decode(monkeypatch):
    """decode = 'device' with a stand-in decoder (CPU tensors, which no batch path reads, so they are downloaded for the loop): the
    download decision and the route are ONE decision.  The `== 1` below is the one assertion of this file that the code before the
    consolidation of generate() does not meet (it asked twice: once to decide the download, once to route)."""
    import torch
    from ssd_keras_amd.data_generator import jpeg_decode
    decoded = []

    def decode_jpeg_batch(sources, device=None, index=None):
        decoded.append(list(sources))
        return [torch.full((4, 5, 3), VALUES[int(s[-1])], dtype=torch.uint8) for s in sources]
    monkeypatch.setattr(jpeg_decode, "decode_jpeg_batch", decode_jpeg_batch)
    calls = _spy(monkeypatch)
    g = _generator()
    g.images, g.decode = None, 'device'
    gen = g.generate(batch_size=2, shuffle=False, transformations=_stubs(), returns={'processed_images', 'original_images'})
    images, originals = next(gen)
    assert decoded == [['file0', 'file1']]
    _rows(images, [_after(10)])                                         # file1 has no ground truth
    assert len(originals) == 1 and isinstance(originals[0], np.ndarray) and int(originals[0][0, 0, 0]) == 10
    assert len(calls) >= 1
    assert len(calls) == 1
