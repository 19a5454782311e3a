"""`SSD7.fused_blocks()` (models/keras_ssd7.py): the plumbing around csrc/ssdhip_convbn.hip -- routing, the cached filter / BatchNorm
tables and their invalidation, train() mode, HIP-graph capture -- on a small model whose maps (76 x 68 -> 38 x 34 -> 19 x 17 -> 9 x 8 ->
4 x 4 -> 2 x 2 -> 1 x 1) put odd sizes in front of the 'valid' pools.  The kernel's arithmetic is tests/test_conv_bn_elu_gpu.py's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE, BATCH = (76, 68, 3), 3


def _model(seed, dtype=None):
    """SSD7 with non-trivial BatchNorm statistics (some gamma negative), eval mode, on the GPU; float32 unless `dtype` is given."""
    import torch
    from ssd_keras_amd.models.keras_ssd7 import build_model
    torch.manual_seed(seed)
    model = build_model(SIZE, 3, mode="training", normalize_coords=True, subtract_mean=127.5, divide_by_stddev=127.5)
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for conv, bn in zip(model.convs, model.bns):
            n = bn.num_features
            conv.bias.copy_(torch.randn(n, generator=g) * 0.2)
            bn.running_mean.copy_(torch.randn(n, generator=g) * 0.3)
            bn.running_var.copy_(torch.rand(n, generator=g) * 1.5 + 0.5)
            bn.weight.copy_((torch.rand(n, generator=g) * 0.8 + 0.6) * torch.where(torch.rand(n, generator=g) < 0.3, -1.0, 1.0))
            bn.bias.copy_(torch.randn(n, generator=g) * 0.3)
    model = model.cuda().to(memory_format=torch.channels_last).eval()
    return model.to(dtype) if dtype is not None else model


def _images(seed=1):
    import torch
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, size=(BATCH,) + SIZE).astype(np.float32)).cuda()


def _hand_chain(model, x):
    """The seven blocks chained by hand from the module's own tensors: tables in float64 on the host, rounded once."""
    import torch
    from ssd_keras_amd import _native as nat
    feats = []
    for i, (conv, bn) in enumerate(zip(model.convs, model.bns)):
        f64 = lambda t: t.detach().double().cpu()
        scale = f64(bn.weight) / torch.sqrt(f64(bn.running_var) + bn.eps)
        shift = f64(bn.bias) + (f64(conv.bias) - f64(bn.running_mean)) * scale
        x = nat.conv_bn_elu(x, nat.conv_bn_elu_pack(conv.weight), scale.float().cuda(), shift.float().cuda(), 5 if i == 0 else 3, pool=i < 3)
        if i >= 3:
            feats.append(x)
            if i < 6:
                x = nat.bias_act_maxpool(x, None, 2, 2, 0, False, relu=False)
    return feats


def _same(a, b):
    import torch
    return len(a) == len(b) and all(s.shape == t.shape and torch.equal(s, t) for s, t in zip(a, b))


def test_features_equal_the_hand_chain_and_follow_their_tensors():
    import torch
    model = _model(3, torch.bfloat16).fused_blocks()
    assert model.fused_blocks() is model
    with torch.no_grad():
        x = model.preprocess(_images()).to(torch.bfloat16)
        feats = model.features(x)
        assert [tuple(f.shape[1:]) for f in feats] == [(64, 9, 8), (48, 4, 4), (48, 2, 2), (32, 1, 1)]
        assert _same(feats, _hand_chain(model, x))
        default = model.fused_blocks(False).features(x)
        assert not _same(feats, default)                 # one rounding per block instead of three: another path really ran
        model.fused_blocks()
        # the stale-cache check: in-place changes of a BatchNorm statistic and of a filter, then another model's state
        model.bns[2].running_mean.add_(0.25)
        model.convs[4].weight.mul_(1.5)
        changed = model.features(x)
        assert not _same(changed, feats) and _same(changed, _hand_chain(model, x))
        model.load_state_dict(_model(4, torch.bfloat16).state_dict())
        loaded = model.features(x)
        assert not _same(loaded, changed) and _same(loaded, _hand_chain(model, x))


def test_switch_off_and_train_mode_keep_the_default_path():
    import torch
    img = _images()
    with torch.no_grad():
        untouched = _model(3, torch.bfloat16)
        want = untouched(img)
        model = _model(3, torch.bfloat16)
        on = model.fused_blocks()(img)
        # shape, anchor and variance columns do not depend on the path
        assert on.shape == want.shape and torch.equal(on[:, :, -8:], want[:, :, -8:])
        assert not torch.equal(on, want)
        assert torch.equal(model.fused_blocks(False)(img), want)
        # train(): BatchNorm uses batch statistics -- the switch must not route around that (and the running statistics move as before)
        a, b = _model(3, torch.bfloat16).train(), _model(3, torch.bfloat16).fused_blocks().train()
        assert torch.equal(a(img), b(img))
        assert all(torch.equal(m.running_mean, n.running_mean) for m, n in zip(a.bns, b.bns))


def test_graphed_replays_equal_eager():
    import torch
    img = _images()
    with torch.no_grad():
        model = _model(3, torch.bfloat16).fused_blocks()
        want = model(img).clone()
        step = model.graphed(img)
        for _ in range(3):
            assert torch.equal(step(img), want)
        # a parameter update between replays reaches the tables the graph reads
        model.bns[0].running_var.mul_(1.3)
        want2 = model(img).clone()
        assert not torch.equal(want2, want) and torch.equal(step(img), want2)


def test_not_farther_from_float32_than_the_default_bf16_path():
    """Against the same weights in float32 on the framework's operators, the largest absolute difference of the loc columns and of the
    softmax columns: the default bf16 path sets the yardstick, the fused path may exceed it by at most a factor of two (it rounds once
    per block where the default rounds three times; the factor covers the run-to-run difference of MIOpen's algorithm choice).
    Measured on an MI355X (printed before the assertion): default path softmax 0.0200, loc 0.1245; fused blocks softmax 0.0136,
    loc 0.0631."""
    import torch
    img = _images()
    with torch.no_grad():
        ref = _model(3)
        ref.fused_inference = False
        want = ref(img)
        model = _model(3, torch.bfloat16)
        default, fused = model(img).float(), model.fused_blocks()(img).float()
    c = want.shape[2] - 12
    err = lambda got, cols: float((got[:, :, cols] - want[:, :, cols]).abs().max())
    conf_d, loc_d = err(default, slice(0, c)), err(default, slice(c, c + 4))
    conf_f, loc_f = err(fused, slice(0, c)), err(fused, slice(c, c + 4))
    print("max |bf16 - float32|: default softmax %.4g loc %.4g; fused blocks softmax %.4g loc %.4g" % (conf_d, loc_d, conf_f, loc_f))
    assert conf_f <= 2 * conf_d and loc_f <= 2 * loc_d
