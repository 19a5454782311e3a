"""`models.resample_classes` on the device: its parameters against the file route's (`resample_keras_weights` on a file of the model,
loaded into a fresh model), for SSD7 and SSD300, bf16 and float32, a class list and an up-sampling integer; then the paths that keep
state DERIVED from the parameters -- packed head images, BatchNorm tables, captured graphs, optimizer masters -- on a resampled model
against a model built fresh from the resampled file, bit for bit: a stale copy of any of them would give other numbers without an error.
And `sample_tensors` on CUDA tensors against its CPU tensor form."""
import hashlib
import itertools
import json
import os

import numpy as np
import pytest

from tests.test_ssd7_fused_training_gpu import deterministic_convolutions  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_SOURCE = 6                                       # classes of the source models, background included
KEEP = [0, 2, 4]
UP = 8


def state_digest():
    name, key, pos, has_gauss, cached = np.random.get_state()
    return hashlib.sha256(key.tobytes() + repr((name, int(pos), int(has_gauss), float(cached))).encode()).hexdigest()


def _build(which, n_classes, mode="training", seed=0):
    """On the host, float32; `_place` moves it."""
    import torch
    torch.manual_seed(seed)
    if which == "ssd7":
        from ssd_keras_amd.models.keras_ssd7 import build_model
        return build_model((64, 64, 3), n_classes, mode=mode, normalize_coords=True, subtract_mean=127.5, divide_by_stddev=127.5)
    from ssd_keras_amd import synthetic as syn
    from ssd_keras_amd.models.keras_ssd300 import ssd_300
    cfg = syn.SSD300_VOC
    return ssd_300((300, 300, 3), n_classes, mode=mode, scales=cfg["scales"], aspect_ratios_per_layer=cfg["aspect_ratios_per_layer"],
                   steps=cfg["steps"], offsets=cfg["offsets"])


def _place(model, dtype):
    import torch
    return model.cuda().to(memory_format=torch.channels_last).eval().to(getattr(torch, dtype))


def _source(which, dtype, mode="training"):
    """An N_SOURCE-class model with distinct head biases and BatchNorm statistics (construction leaves zeros and ones)."""
    import torch
    model = _build(which, N_SOURCE - 1, mode=mode, seed=3)
    g = torch.Generator().manual_seed(103)
    with torch.no_grad():
        for m in list(model.conf_heads) + list(model.loc_heads):
            m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.5)
        for m in model.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.copy_(torch.randn(m.num_features, generator=g) * 0.3)
                m.running_var.copy_(torch.rand(m.num_features, generator=g) * 1.5 + 0.5)
                m.weight.copy_(torch.rand(m.num_features, generator=g) * 0.8 + 0.6)
                m.bias.copy_(torch.randn(m.num_features, generator=g) * 0.3)
    return _place(model, dtype)


@pytest.fixture(scope="module")
def source_files(tmp_path_factory):
    """(which, dtype, mode) -> (the source model, the path of its weight file); built on first use, shared, never modified."""
    from ssd_keras_amd.models.keras_weights import save_keras_weights_h5
    root, made = tmp_path_factory.mktemp("resample_gpu"), {}

    def get(which, dtype, mode="training"):
        key = (which, dtype, mode)
        if key not in made:
            model = _source(which, dtype, mode)
            path = str(root / ("%s_%s_%s.h5" % key))
            save_keras_weights_h5(model, path)
            made[key] = (model, path)
        return made[key]
    return get


def _from_file(which, dtype, src, classes, tmp_path, mode="training", **kw):
    """The file route: resample the file, build a model for the new number of classes, load the file."""
    from ssd_keras_amd.models.keras_weights import load_keras_weights, resample_keras_weights
    dst = str(tmp_path / "resampled.h5")
    resample_keras_weights(src, dst, N_SOURCE, classes, **kw)
    n_new = classes if isinstance(classes, int) else len(classes)
    fresh = _place(_build(which, n_new - 1, mode=mode, seed=9), dtype)
    loaded, missing = load_keras_weights(fresh, dst, strict_shapes=True)
    assert missing == []
    return fresh


def _images(size, seed=1, batch=2):
    import torch
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, size=(batch, size, size, 3)).astype(np.float32)).cuda()


@pytest.mark.parametrize("classes", [KEEP, UP], ids=["list", "upsample"])
@pytest.mark.parametrize("dtype", ["bfloat16", "float32"])
@pytest.mark.parametrize("which", ["ssd7", "ssd300"])
def test_parameters_equal_the_file_route(source_files, tmp_path, which, dtype, classes):
    import torch
    from ssd_keras_amd.models import resample_classes
    source, src = source_files(which, dtype)
    kept = {k: v.clone() for k, v in source.state_dict().items()}
    np.random.seed(11)
    fresh = _from_file(which, dtype, src, classes, tmp_path)
    state = state_digest()
    np.random.seed(11)
    live = resample_classes(source, classes)
    assert state_digest() == state
    n_new = classes if isinstance(classes, int) else len(classes)
    assert type(live) is type(source) and live is not source and live.n_classes == n_new and not live.training
    sa, sb, so = live.state_dict(), fresh.state_dict(), source.state_dict()
    assert list(sa) == list(sb) == list(so)
    for k in sa:
        assert sa[k].dtype == sb[k].dtype and sa[k].device == sb[k].device == so[k].device and torch.equal(sa[k], sb[k]), k
        if not k.startswith("conf_heads."):
            assert torch.equal(sa[k], kept[k]) and (sa[k].data_ptr() != so[k].data_ptr() or sa[k].numel() == 0), k
    for p, q in zip(live.parameters(), source.parameters()):
        assert p.dtype == q.dtype == getattr(torch, dtype) and p.requires_grad == q.requires_grad
        if p.shape == q.shape:
            assert p.stride() == q.stride()
    head = live.conf_heads[1].weight
    assert head.shape[0] == source.conf_heads[1].weight.shape[0] // N_SOURCE * n_new
    assert head.is_contiguous(memory_format=torch.channels_last) and source.conf_heads[1].weight.is_contiguous(memory_format=torch.channels_last)
    if isinstance(classes, int):                        # new kernel channels are drawn, new bias entries zero
        assert int((live.conf_heads[0].bias == 0).sum()) == live.conf_heads[0].bias.numel() // UP * (UP - N_SOURCE)
        assert float(live.conf_heads[0].weight.detach().float().abs().min()) > 0
    # the source model is what it was
    assert all(torch.equal(v, kept[k]) for k, v in source.state_dict().items())


def _stale_state_check(which, source_files, tmp_path, prepare):
    import torch
    from ssd_keras_amd.models import resample_classes
    source, src = source_files(which, "bfloat16", "inference")
    images = _images(300 if which == "ssd300" else 64)
    with torch.no_grad():
        prepare(source)
        seen = source.graphed(images.clone())(images).clone()        # the source has its derived tensors built, and a captured graph
        live = prepare(resample_classes(source, KEEP))
        fresh = prepare(_from_file(which, "bfloat16", src, KEEP, tmp_path, mode="inference"))
        want = fresh(images).clone()
        got_graph = live.graphed(images.clone())(images).clone()
        want_graph = fresh.graphed(images.clone())(images).clone()
        got = live(images).clone()
        again = source(images).clone()
    assert want.shape == got.shape == got_graph.shape and want.shape[-1] == 6 and bool((want[..., 1] > 0).any())
    assert set(want[..., 0].unique().tolist()) <= {0.0, 1.0, 2.0}              # class ids of a 3-class model
    assert torch.equal(got_graph, want_graph) and torch.equal(got, want) and torch.equal(got_graph, want)
    assert torch.equal(again, seen) and not torch.equal(seen, want)


def test_graphed_fused_inference_of_a_resampled_ssd300(source_files, tmp_path):
    """bf16 SSD300 in 'inference' mode: the fused path with the packed heads and the decode from the heads, eager and as a captured
    graph, on the resampled model == on a model built fresh from the resampled file."""
    _stale_state_check("ssd300", source_files, tmp_path, lambda m: m)


def test_graphed_fused_blocks_of_a_resampled_ssd7(source_files, tmp_path):
    _stale_state_check("ssd7", source_files, tmp_path, lambda m: m.fused_blocks())


def test_two_training_steps_on_a_resampled_ssd7(source_files, tmp_path, deterministic_convolutions):  # noqa: F811
    """fit_generator(graph=True) on the resampled bf16 SSD7, every training route in libssdhip, SGD with float32 masters, labels from an
    SSDInputEncoder of the new class count: finite loss, the conf heads' masters move, and loss, parameters, buffers and optimizer
    state equal those of the same two steps on the model built fresh from the resampled file."""
    import torch
    from ssd_keras_amd import synthetic as syn
    from ssd_keras_amd.keras_loss_function.keras_ssd_loss import SSDLoss
    from ssd_keras_amd.models import resample_classes
    from ssd_keras_amd.optimizers import SGD
    from ssd_keras_amd.ssd_encoder_decoder.ssd_input_encoder import SSDInputEncoder
    from ssd_keras_amd.training import fit_generator
    source, src = source_files("ssd7", "bfloat16")
    live = resample_classes(source, KEEP)
    fresh = _from_file("ssd7", "bfloat16", src, KEEP, tmp_path)
    encoder = SSDInputEncoder(64, 64, live.n_classes - 1, live.predictor_sizes(), min_scale=0.1, max_scale=0.9,
                              aspect_ratios_global=[0.5, 1.0, 2.0], variances=[1.0, 1.0, 1.0, 1.0], normalize_coords=True)
    labels = [encoder(syn.make_ground_truth(2, live.n_classes - 1, 64, 64, max_boxes=4, seed=20 + k)) for k in range(2)]
    assert labels[0].shape[2] == 3 + 12 and labels[0][..., 1:3].any()
    batches = [(_images(64, seed=10 + k), torch.from_numpy(y.astype(np.float32)).cuda()) for k, y in enumerate(labels)]

    def run(model):
        model.train().fused_blocks(True, training=True, convolutions=True, heads=True)
        start = [h.weight.detach().float().clone() for h in model.conf_heads]
        opt = SGD(model.parameters(), lr=1e-2, momentum=0.9, master_weights=True)
        # n_neg_min beyond the 2 x 340 anchors: every anchor is in the loss, so every head -- the 1 x 1 map's four anchors too, which
        # hard-negative mining alone may pass over -- has a gradient
        hist = fit_generator(model, itertools.cycle(batches), 2, 1, optimizer=opt, loss=SSDLoss(neg_pos_ratio=3, n_neg_min=1000, alpha=1.0), graph=True)
        return opt, hist, start

    opt_a, hist_a, start = run(live)
    opt_b, hist_b, _ = run(fresh)
    print("loss after two steps: resampled model %r, fresh from the file %r" % (hist_a.history["loss"], hist_b.history["loss"]))
    assert len(hist_a.history["loss"]) == 1 and np.isfinite(hist_a.history["loss"][0]) and hist_a.history == hist_b.history
    assert opt_a.iterations == opt_b.iterations == 2
    for head, was in zip(live.conf_heads, start):
        master = opt_a.state[head.weight]["master"]
        assert master.dtype == torch.float32 and master.shape == was.shape and not torch.equal(master, was)
    sa, sb = live.state_dict(), fresh.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    for p, q in zip(live.parameters(), fresh.parameters()):
        assert set(opt_a.state[p]) == set(opt_b.state[q]) and "master" in opt_a.state[p]
        assert all(torch.equal(opt_a.state[p][k], opt_b.state[q][k]) for k in opt_a.state[p] if torch.is_tensor(opt_a.state[p][k]))
    # the source model took no part in any of it
    assert source.n_classes == N_SOURCE and not source.training and all(int(bn.num_batches_tracked) == 0 for bn in source.bns)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_sample_tensors_on_cuda_tensors(dtype):
    """The golden cases on CUDA tensors: results on the device, bit-identical to the CPU tensor form, same consumption of `np.random`."""
    import torch
    from ssd_keras_amd.misc_utils.tensor_sampling_utils import sample_tensors
    cases = json.load(open(os.path.join(GOLDEN, "tensor_sampling.json")))["cases"]
    dt = getattr(torch, dtype)
    n = 0
    with np.load(os.path.join(GOLDEN, "tensor_sampling.npz")) as z:
        for name, case in sorted(cases.items()):
            inst = case["instructions"]
            if "error" in case or isinstance(inst, dict) or any(isinstance(i, dict) for i in inst):
                continue
            host = [torch.from_numpy(z["%s/in/%d" % (name, i)]).to(dt) for i in range(case["n_inputs"])]
            kw = dict(axes=case["axes"], init=case["init"], mean=case["mean"], stddev=case["stddev"])
            np.random.seed(case["seed"])
            want = sample_tensors(host, inst, **kw)
            state = state_digest()
            np.random.seed(case["seed"])
            got = sample_tensors([t.cuda() for t in host], inst, **kw)
            assert state_digest() == state, name
            assert len(got) == len(want)
            for g, w in zip(got, want):
                assert g.is_cuda and g.dtype == dt and torch.equal(g.cpu(), w), name
            n += 1
    assert n >= 20
    with pytest.raises(TypeError):
        sample_tensors([host[0].cuda(), np.zeros(3, np.float32)], [1], axes=[[0]])
