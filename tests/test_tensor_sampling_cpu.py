"""misc_utils.tensor_sampling_utils.sample_tensors against the reference's recorded results (tests/golden/tensor_sampling.npz / .json,
written by tests/golden/make_tensor_sampling_golden.py from the live reference), its torch form against its array form, the file route
`resample_keras_weights`, and what the resampled classifier computes (the class relation, in float64)."""
import ast
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
GEN = os.path.join(GOLDEN, "make_h5_golden.py")
CONDA = "/opt/conda/bin/python3.9"
sys.path.insert(0, GOLDEN)
sys.path.insert(0, HERE)

MANIFEST = json.load(open(os.path.join(GOLDEN, "tensor_sampling.json")))
CASES = MANIFEST["cases"]
PASSING = sorted(n for n, c in CASES.items() if "error" not in c)


def _real_h5py():
    if not os.path.exists(CONDA):
        return False
    try:
        return subprocess.run([CONDA, "-c", "import h5py"], capture_output=True, timeout=120).returncode == 0
    except Exception:
        return False


def state_digest():
    name, key, pos, has_gauss, cached = np.random.get_state()
    return hashlib.sha256(key.tobytes() + repr((name, int(pos), int(has_gauss), float(cached))).encode()).hexdigest()


def decode(inst):
    if isinstance(inst, dict) and "numpy_integer" in inst:
        return np.int64(inst["numpy_integer"])
    if isinstance(inst, dict) and "tuple" in inst:
        return tuple(decode(i) for i in inst["tuple"])
    if isinstance(inst, list):
        return [decode(i) for i in inst]
    return inst


@pytest.fixture(scope="module")
def arrays():
    with np.load(os.path.join(GOLDEN, "tensor_sampling.npz")) as z:
        return {k: z[k] for k in z.files}


def _call(case, inputs):
    from ssd_keras_amd.misc_utils.tensor_sampling_utils import sample_tensors
    np.random.seed(case["seed"])
    return sample_tensors(inputs, decode(case["instructions"]), axes=case["axes"], init=case["init"], mean=case["mean"], stddev=case["stddev"])


def _inputs(arrays, name):
    return [arrays["%s/in/%d" % (name, i)].copy() for i in range(CASES[name]["n_inputs"])]


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_case(arrays, name):
    """Values, dtypes and the state of the global `np.random` stream after the call, bit for bit; the errors by type -- and the stream
    after them, since an unknown `init` of a later tensor is only met after the draws in front of it."""
    case = CASES[name]
    inputs = _inputs(arrays, name)
    kept = [a.copy() for a in inputs]
    if "error" in case:
        with pytest.raises(Exception) as e:
            _call(case, inputs)
        assert type(e.value).__name__ == case["error"] == "ValueError"
    else:
        outs = _call(case, inputs)
        assert isinstance(outs, list) and len(outs) == len(case["out_dtypes"])
        for i, o in enumerate(outs):
            want = arrays["%s/out/%d" % (name, i)]
            assert isinstance(o, np.ndarray) and str(o.dtype) == case["out_dtypes"][i] == str(want.dtype), (name, i)
            assert o.shape == want.shape and o.tobytes() == np.ascontiguousarray(want).tobytes(), (name, i)
            assert not any(np.shares_memory(o, a) for a in inputs)
    assert state_digest() == case["state"], name
    assert all(np.array_equal(a, b) for a, b in zip(inputs, kept))


def test_golden_covers_what_it_should():
    ups = [n for n in PASSING if "upsample" in n]
    assert len(PASSING) >= 20 and len(CASES) - len(PASSING) >= 8 and len(ups) >= 8
    assert all(CASES[n]["out_dtypes"][0] == "float64" for n in ups)
    # an up-sampled float32 input comes back float64, a sub-sampled one keeps its dtype
    assert CASES["upsample_init_none"]["out_dtypes"] == ["float64", "float64"] and CASES["int_subsample"]["out_dtypes"] == ["float32", "float32"]


def test_signature_is_the_reference_s():
    import api_surface
    from ssd_keras_amd.misc_utils import tensor_sampling_utils as tsu
    got = api_surface.extract(os.path.dirname(os.path.dirname(tsu.__file__)), {"misc_utils/tensor_sampling_utils.py": ["sample_tensors"]})
    got = json.loads(json.dumps(got))
    assert got == MANIFEST["signature"]
    assert [p for p, _ in got["misc_utils/tensor_sampling_utils.py"]["sample_tensors"]] == [
        "weights_list", "sampling_instructions", "axes", "init", "mean", "stddev"]
    assert ast.parse(open(tsu.__file__).read())                       # (the file the signature was read from)


@pytest.mark.parametrize("dtype", ["float32", "float64", "bfloat16", "float16"])
@pytest.mark.parametrize("name", PASSING)
def test_tensor_form_on_cpu_equals_array_form(arrays, name, dtype):
    """Same selection, same draws: the tensor result is the array result rounded ONCE to the inputs' dtype (for a Gaussian fill: the
    float64 draw -> that dtype), and the stream ends where the array form leaves it."""
    import torch
    case = CASES[name]
    dt = getattr(torch, dtype)
    tensors = [torch.from_numpy(a).to(dt) for a in _inputs(arrays, name)]
    kept = [t.clone() for t in tensors]
    as_arrays = [t.to(torch.float64 if dtype == "float64" else torch.float32).numpy() for t in tensors]   # exact
    want = _call(case, as_arrays)
    state = state_digest()
    got = _call(case, tensors)
    assert state_digest() == state
    assert isinstance(got, list) and len(got) == len(want)
    for g, w, t in zip(got, want, tensors):
        assert torch.is_tensor(g) and g.dtype == dt and g.device == t.device and tuple(g.shape) == w.shape
        assert torch.equal(g, torch.from_numpy(np.ascontiguousarray(w)).to(dt))
        assert g.data_ptr() != t.data_ptr()
    assert all(torch.equal(a, b) for a, b in zip(tensors, kept))


def test_tensor_form_errors_and_mixing(arrays):
    import torch
    from ssd_keras_amd.misc_utils.tensor_sampling_utils import sample_tensors
    for name, case in CASES.items():
        if "error" in case:
            with pytest.raises(ValueError):
                _call(case, [torch.from_numpy(a) for a in _inputs(arrays, name)])
            assert state_digest() == case["state"], name
    k, b = _inputs(arrays, "list_last_axis")
    for mixed in ([k, torch.from_numpy(b)], [torch.from_numpy(k), b]):
        with pytest.raises(TypeError):
            sample_tensors(mixed, [3, 3, 4, [0, 1]], axes=[[3]])


# ------------------------------------------------------------------------------------------------------------------------------------------
# the file route
# ------------------------------------------------------------------------------------------------------------------------------------------
N_SOURCE = 6                                     # classes of the synthetic checkpoints, background included (81 in the tutorial's)


def _ssd300(n_classes, seed=0):
    import torch
    from ssd_keras_amd import synthetic as syn
    from ssd_keras_amd.models.keras_ssd300 import ssd_300
    cfg = syn.SSD300_VOC
    torch.manual_seed(seed)
    return ssd_300((300, 300, 3), n_classes, mode="training", scales=cfg["scales"], aspect_ratios_per_layer=cfg["aspect_ratios_per_layer"],
                   steps=cfg["steps"], offsets=cfg["offsets"])


def _ssd7(n_classes, seed=0, size=(64, 64, 3)):
    import torch
    from ssd_keras_amd.models.keras_ssd7 import build_model
    torch.manual_seed(seed)
    return build_model(size, n_classes, mode="training", normalize_coords=True, subtract_mean=127.5, divide_by_stddev=127.5)


def _randomize_heads(model, seed):
    """Biases are zero and BatchNorm statistics trivial after construction: give every conf / loc head and BatchNorm distinct values."""
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in list(model.conf_heads) + list(model.loc_heads):
            m.bias.copy_(torch.randn(m.bias.shape, generator=g))
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) + 0.5)
    return model


BUILDERS = {"ssd300": _ssd300, "ssd7": _ssd7}
N_HEADS = {"ssd300": 6, "ssd7": 4}


@pytest.fixture(scope="module")
def checkpoints(tmp_path_factory):
    """{layout: (path of an N_SOURCE-class weight file in that layout, its arrays)} -- written once, read-only for the tests."""
    from ssd_keras_amd.models.keras_weights import _read_h5, save_keras_weights_h5
    out = {}
    for which, make in BUILDERS.items():
        path = str(tmp_path_factory.mktemp("resample") / (which + "_source.h5"))
        save_keras_weights_h5(_randomize_heads(make(N_SOURCE - 1), 5), path, backend="theano", keras_version="2.1.6")
        out[which] = (path, _read_h5(path))
    return out


def _attrs(path):
    from ssd_keras_amd.models.keras_weights import _read_h5_attrs
    return _read_h5_attrs(path)


def _classifiers(which, weights):
    names = [n for n in weights if n.endswith("_mbox_conf") or (n.startswith("classes") and n[7:].isdigit())]
    assert len(names) == N_HEADS[which]
    return names


@pytest.mark.parametrize("which", ["ssd300", "ssd7"])
def test_resample_file_with_a_class_list(checkpoints, tmp_path, which):
    import torch
    from ssd_keras_amd.models.keras_weights import _read_h5, export_keras_weights, load_keras_weights, resample_keras_weights
    src, weights = checkpoints[which]
    if which == "ssd300":
        assert weights["conv4_3_norm_mbox_conf"][0].shape == (3, 3, 512, 4 * N_SOURCE) and weights["fc7_mbox_conf"][0].shape == (3, 3, 1024, 6 * N_SOURCE)
    dst = str(tmp_path / "dst.h5")
    classes = [0, 4, 2]
    before = state_digest()
    changed = resample_keras_weights(src, dst, N_SOURCE, classes)
    assert state_digest() == before                                    # an index list draws nothing
    got = _read_h5(dst)
    names = _classifiers(which, weights)
    assert list(changed) == names and list(got) == list(weights)
    for name in weights:
        if name in names:
            kernel, bias = weights[name]
            n_boxes = kernel.shape[3] // N_SOURCE
            idx = [c + i * N_SOURCE for i in range(n_boxes) for c in classes]
            assert changed[name] == (n_boxes * N_SOURCE, n_boxes * 3)
            assert got[name][0].dtype == kernel.dtype and np.array_equal(got[name][0], kernel[:, :, :, idx])
            assert got[name][1].dtype == bias.dtype and np.array_equal(got[name][1], bias[idx]) and np.any(bias[idx] != 0)
        else:
            assert len(got[name]) == len(weights[name])
            assert all(a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes() for a, b in zip(got[name], weights[name])), name
    assert _attrs(dst) == _attrs(src) and _attrs(dst)[2:] == ("theano", "2.1.6")
    model = BUILDERS[which](2, seed=1)
    loaded, missing = load_keras_weights(model, dst, strict_shapes=True)
    assert missing == [] and sorted(loaded) == sorted(weights)
    back = export_keras_weights(model)
    assert all(np.array_equal(a, b) for name in got for a, b in zip(back[name], got[name]))
    assert model.n_classes == 3 and torch.is_tensor(model.conf_heads[0].weight)


@pytest.mark.parametrize("which", ["ssd300", "ssd7"])
def test_resample_file_with_an_integer(checkpoints, tmp_path, which):
    """Up-sampling 6 -> 8 classes: the old channels sit at the seed's positions (channel 0 first), the new kernel channels are the
    seed's Gaussian draws rounded once to float32, the new bias entries zero; sub-sampling 6 -> 3 keeps channel 0 and the seed's choice."""
    from ssd_keras_amd.models.keras_weights import _read_h5, load_keras_weights, resample_keras_weights
    src, weights = checkpoints[which]
    names = _classifiers(which, weights)
    up, down = str(tmp_path / "up.h5"), str(tmp_path / "down.npz")
    np.random.seed(77)
    changed = resample_keras_weights(src, up, N_SOURCE, 8, stddev=0.25, mean=-1.0)
    after = state_digest()
    got = _read_h5(up)
    np.random.seed(77)
    for name in names:
        kernel, bias = weights[name]
        old, new = kernel.shape[3], int(8 * kernel.shape[3] / N_SOURCE)
        fill = np.random.normal(loc=-1.0, scale=0.25, size=kernel.shape[:3] + (new,))
        at = np.concatenate([[0], np.sort(np.random.choice(np.arange(1, new), old - 1, replace=False))])
        rest = np.setdiff1d(np.arange(new), at)
        assert changed[name] == (old, new) and got[name][0].dtype == np.float32 and got[name][1].dtype == np.float32
        assert np.array_equal(got[name][0][..., at], kernel) and np.array_equal(got[name][0][..., rest], fill[..., rest].astype(np.float32))
        assert np.array_equal(got[name][1][at], bias) and not got[name][1][rest].any()
    assert state_digest() == after
    load_keras_weights(BUILDERS[which](7, seed=1), up, strict_shapes=True)

    np.random.seed(78)
    changed = resample_keras_weights(src, down, N_SOURCE, 3, classifier_names=names[:2])
    from ssd_keras_amd.models.keras_weights import _read_npz
    got = _read_npz(down)
    np.random.seed(78)
    for name in names[:2]:
        kernel, bias = weights[name]
        old = kernel.shape[3]
        idx = np.concatenate([[0], np.sort(np.random.choice(np.arange(1, old), old // 2 - 1, replace=False))])
        assert changed[name] == (old, old // 2)
        assert np.array_equal(got[name][0], kernel[..., idx]) and np.array_equal(got[name][1], bias[idx])
    assert list(changed) == names[:2] and all(np.array_equal(got[n][0], weights[n][0]) for n in names[2:])


def test_resample_file_refusals(checkpoints, tmp_path):
    from ssd_keras_amd.models.keras_weights import resample_keras_weights
    src, weights = checkpoints["ssd7"]
    dst = str(tmp_path / "dst.h5")
    with pytest.raises(ValueError, match="classes4"):
        resample_keras_weights(src, dst, 5, [0, 1])                        # 4 boxes x 6 classes = 24 channels: no multiple of 5
    with pytest.raises(ValueError, match="no_such_layer"):
        resample_keras_weights(src, dst, N_SOURCE, [0, 1], classifier_names=["classes4", "no_such_layer"])
    with pytest.raises(ValueError, match="bn1"):
        resample_keras_weights(src, dst, N_SOURCE, [0, 1], classifier_names=["bn1"])
    assert not os.path.exists(dst)
    for same in (src, os.path.join(os.path.dirname(src), ".", os.path.basename(src))):
        with pytest.raises(ValueError, match="source"):
            resample_keras_weights(src, same, N_SOURCE, [0, 1])
    from ssd_keras_amd.models.keras_weights import _read_h5
    assert all(np.array_equal(a, b) for n, ws in _read_h5(src).items() for a, b in zip(ws, weights[n]))


@pytest.mark.parametrize("name", ["ssd7_model_save_h5py2.h5", "ssd7_save_weights_h5py3.h5", "ssd300_save_weights_h5py2.h5"])
def test_resample_files_of_the_real_library(tmp_path, name):
    """Files the real HDF5 library wrote in Keras' layout (tests/golden/h5): a `model.save()` file's `model_weights` group, both
    attribute styles, the weightless layers Keras lists in `layer_names` -- all handed on as found."""
    import make_h5_golden as gen
    from ssd_keras_amd.models.keras_weights import _read_h5, resample_keras_weights
    src = os.path.join(GOLDEN, "h5", name)
    n_source = 3 if name.startswith("ssd300") else 6
    layers = gen.ssd300_layers() if name.startswith("ssd300") else gen.ssd7_layers()
    dst = str(tmp_path / "dst.h5")
    changed = resample_keras_weights(src, dst, n_source, [0, 2])
    weights, got = _read_h5(src), _read_h5(dst)
    assert len(changed) == (6 if name.startswith("ssd300") else 4)
    layer_names, weight_names, backend, version = _attrs(dst)
    assert layer_names == [n for n, _ in layers] and len(layer_names) > len(weights)
    assert weight_names == {n: [w for w, _, _ in ws] for n, ws in layers} and (backend, version) == ("tensorflow", "2.2.4")
    assert list(got) == list(weights)
    for lname in weights:
        if lname in changed:
            idx = [c + i * n_source for i in range(changed[lname][0] // n_source) for c in (0, 2)]
            assert np.array_equal(got[lname][0], weights[lname][0][..., idx]) and np.array_equal(got[lname][1], weights[lname][1][idx])
        else:
            assert all(a.tobytes() == b.tobytes() and a.dtype == b.dtype for a, b in zip(got[lname], weights[lname]))


@pytest.mark.skipif(not _real_h5py(), reason="the Anaconda interpreter with h5py is not in this image")
def test_the_real_library_opens_the_resampled_file(checkpoints, tmp_path):
    from ssd_keras_amd.models.keras_weights import _read_h5_lite, resample_keras_weights
    for src, dst in ((checkpoints["ssd7"][0], str(tmp_path / "a.h5")), (os.path.join(GOLDEN, "h5", "ssd7_model_save_h5py2.h5"), str(tmp_path / "b.h5"))):
        np.random.seed(3)
        resample_keras_weights(src, dst, N_SOURCE, 9)
        r = subprocess.run([CONDA, GEN, "--dump", dst], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        seen = json.loads(r.stdout)
        ours = _read_h5_lite(dst)
        layer_names, weight_names, backend, version = _attrs(dst)
        assert seen["attrs"]["/"]["layer_names"] == layer_names and seen["attrs"]["/"]["backend"] == backend
        assert seen["attrs"]["/"]["keras_version"] == version
        n = 0
        for lname, arrs in ours.items():
            assert seen["attrs"]["/" + lname]["weight_names"] == weight_names[lname]
            for wname, a in zip(weight_names[lname], arrs):
                info = seen["datasets"]["/%s/%s" % (lname, wname)]
                assert info["shape"] == list(a.shape) and info["sha1"] == hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()
                n += 1
        assert n == len(seen["datasets"]) == 58
        assert seen["datasets"]["/classes4/classes4/kernel:0"]["shape"][3] == 4 * 9
        for lname in layer_names:
            if lname not in ours:
                assert seen["attrs"]["/" + lname]["weight_names"] == []


# ------------------------------------------------------------------------------------------------------------------------------------------
# the live model
# ------------------------------------------------------------------------------------------------------------------------------------------
def test_class_relation_in_float64():
    """SSD7 at 64 x 64, 5 source classes, keep [0, 2, 4]: the kept classes' logits are the same float64 dot products (at most
    9 x 64 terms) in both models, so the new model's class probabilities are the source model's probabilities of the kept classes
    divided by their sum, up to rounding of order 1e-13; 1e-9 leaves four orders of margin and cannot hide a wrong channel.  The loc and
    anchor columns do not depend on the classes at all.  (`forward` itself returns float32 -- its softmax takes a float32 copy of the
    logits -- so the 1e-9 statement is made on the float64 graph put together from the models' own layers, and `forward` is checked
    beside it at float32's precision.)"""
    import torch
    from ssd_keras_amd.models import resample_classes
    keep = [0, 2, 4]
    source = _randomize_heads(_ssd7(4, seed=2), 6).double().train()
    kept = {k: v.clone() for k, v in source.state_dict().items()}
    before = state_digest()
    new = resample_classes(source, keep)
    assert state_digest() == before
    assert type(new) is type(source) and new.n_classes == 3 and new.training and new is not source
    assert all(p.dtype == torch.float64 for p in new.parameters())
    assert all(torch.equal(v, kept[k]) for k, v in source.state_dict().items())
    images = torch.from_numpy(np.random.RandomState(1).randint(0, 256, size=(2, 64, 64, 3)).astype(np.float64))
    source.eval(), new.eval()                     # (running statistics: the two forward passes see the same normalisation)

    def float64_predictions(model):
        """`forward` hands its softmax a float32 copy of the logits (models/_common.py, 'mbox_conf_softmax'), whatever the model's
        dtype; the float64 statement of the same graph from the model's own parts: (class probabilities, loc columns)."""
        feats = model.features(model.preprocess(images).double())
        rows = lambda heads, n: torch.cat([h(f).permute(0, 2, 3, 1).reshape(2, -1, n) for h, f in zip(heads, feats)], dim=1)
        return torch.softmax(rows(model.conf_heads, model.n_classes), dim=-1), rows(model.loc_heads, 4)

    with torch.no_grad():
        (pa, la), (pb, lb) = float64_predictions(source), float64_predictions(new)
        a, b = source(images), new(images)
    assert pa.dtype == torch.float64 and pa.shape[2] == 5 and pb.shape[2] == 3 and pa.shape[1] == pb.shape[1] == a.shape[1]
    want = pa[..., keep] / pa[..., keep].sum(dim=-1, keepdim=True)
    err = float((pb - want).abs().max())
    print("class relation in float64: max |difference| %.3g" % err)
    assert err <= 1e-9
    assert float((lb - la).abs().max()) <= 1e-9 and pb.std() > 1e-3
    # ... and through `forward`, whose softmax is float32 over the same (rounded) logits: exponentials, a sum of at most five terms and
    # a division on either side plus the renormalisation here, each a relative rounding of 2^-24 on values <= 1 -> 16 x 2^-24 < 1e-6;
    # the loc and anchor columns are the same numbers
    assert a.shape[2] == 5 + 12 and b.shape[2] == 3 + 12 and a.dtype == torch.float32
    want32 = a[..., keep] / a[..., keep].sum(dim=-1, keepdim=True)
    err32 = float((b[..., :3] - want32).abs().max())
    print("class relation through forward (float32 softmax): max |difference| %.3g" % err32)
    assert err32 <= 1e-6 and torch.equal(b[..., 3:], a[..., 5:])
    # every tensor but the conf heads is equal, and none is shared
    sa, sb = source.state_dict(), new.state_dict()
    assert list(sa) == list(sb)
    for k in sa:
        assert sa[k].data_ptr() != sb[k].data_ptr() or sa[k].numel() == 0
        if k.startswith("conf_heads."):
            assert sb[k].shape[0] * 5 == sa[k].shape[0] * 3
        else:
            assert torch.equal(sa[k], sb[k]), k


def test_live_route_equals_file_route_on_cpu(tmp_path):
    """float32 SSD7 on the CPU (the GPU suite has SSD300 and bf16): resample_classes == resample_keras_weights + load_keras_weights,
    parameters and stream state, for a list, an up-sampling and a sub-sampling integer; switches and caches start afresh."""
    import torch
    from ssd_keras_amd.models import resample_classes
    from ssd_keras_amd.models.keras_weights import load_keras_weights, resample_keras_weights, save_keras_weights_h5
    source = _randomize_heads(_ssd7(4, seed=2), 6).eval().fused_blocks(True)
    source.conf_heads[1].weight.requires_grad_(False)
    source.l2_regularization = 1e-3                                    # set after construction, as training scripts do
    src = str(tmp_path / "src.h5")
    save_keras_weights_h5(source, src)
    for n, classes in enumerate(([0, 3, 1], 8, 2)):
        dst = str(tmp_path / ("dst%d.h5" % n))
        np.random.seed(5)
        resample_keras_weights(src, dst, 5, classes)
        state = state_digest()
        n_new = classes if isinstance(classes, int) else len(classes)
        fresh = _ssd7(n_new - 1, seed=9)
        fresh.load_state_dict({k: v for k, v in source.state_dict().items() if not k.startswith("conf_heads.")}, strict=False)
        load_keras_weights(fresh, dst, strict_shapes=True)
        np.random.seed(5)
        live = resample_classes(source, classes)
        assert state_digest() == state
        sa, sb = live.state_dict(), fresh.state_dict()
        assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) and sa[k].dtype == sb[k].dtype for k in sa)
        assert not live.training and not any(m.training for m in live.modules())
        assert not live.conf_heads[1].weight.requires_grad and live.conf_heads[0].weight.requires_grad
        assert live.l2_regularization == 1e-3 and live.subtract_mean == source.subtract_mean
        assert "_fused_blocks" not in live.__dict__ and live.__dict__.get("_precise") is None and not live._packed_heads
    with pytest.raises(TypeError):
        resample_classes(torch.nn.Conv2d(3, 3, 1), [0, 1])
    with pytest.raises(ValueError):
        resample_classes(source, [0])
